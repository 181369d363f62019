"""csrc/store_plan_core.h (admission of a window of ingested records to the bounded record store: the size of the store for the first of
several windows, and whether the store spills before the window is written) against the two first-window formulas the BGZF ingest and the
SAM text ingest held before they shared one, frozen in tests/c/store_plan_host.cpp, and against the predicate written out here.
The program form of the same file walks the same grid built with -fsanitize=address,undefined."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "c", "store_plan_host.cpp")
LIMIT = 2 ** 32 - 16
CAPS = (50_000, 2 ** 31, 2 ** 32)
SCALES = (1.0001, 1.1, 7.3, 1e6)


def grid():
    for cap in CAPS:
        for have in (0, 1, cap - 1, cap, 2 ** 32 - 17):
            for add in (1, 1000, cap):
                for scale in SCALES:
                    for spare in (0, 1):      # records / the CIGAR column with its spare word
                        yield have, add, spare, scale, cap


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("stplan") / "store_plan_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-o", so, SRC])
    L = C.CDLL(so)
    for f in (L.stplan_size, L.stplan_size_frozen_bgzf, L.stplan_size_frozen_sam):
        f.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_double, C.c_uint64]
        f.restype = C.c_uint64
    L.stplan_past_limit.argtypes = [C.c_uint64, C.c_uint64]
    return L


def test_first_window_size_equals_both_frozen_formulas(host):
    n = 0
    for have, add, spare, scale, cap in grid():
        got = host.stplan_size(have, add, spare, scale, cap)
        assert got == host.stplan_size_frozen_bgzf(have, add, spare, scale, cap), (have, add, spare, scale, cap)
        assert got == host.stplan_size_frozen_sam(have, add, spare, scale, cap), (have, add, spare, scale, cap)
        n += 1
    assert n == 3 * 5 * 3 * 4 * 2


def test_first_window_size_bounds(host):
    """Never less than the window needs; beyond that never past the cap (plus its slack) or the 32-bit limit."""
    seen_scaled = seen_capped = seen_need = 0
    for have, add, spare, scale, cap in grid():
        got, need = host.stplan_size(have, add, spare, scale, cap), have + add + spare
        ceiling = min(cap + 1024, LIMIT)
        assert need <= got <= max(need, ceiling), (have, add, spare, scale, cap)
        whole = have + int(add * scale) + 1024
        seen_scaled += got == whole and need < whole < ceiling
        seen_capped += got == ceiling and need < ceiling
        seen_need += got == need
    assert seen_scaled and seen_capped and seen_need      # all three outcomes occur on the grid


def test_spill_predicate_truth_table(host):
    for empty, mates, fail, over_r, over_c in itertools.product((0, 1), repeat=5):
        want = (not empty) and (not mates) and (not fail) and bool(over_r or over_c)
        assert bool(host.stplan_spill_first(empty, mates, fail, over_r, over_c)) == want, (empty, mates, fail, over_r, over_c)


def test_hard_limit(host):
    assert not host.stplan_past_limit(LIMIT - 2, 1) and host.stplan_past_limit(LIMIT - 1, 1) and host.stplan_past_limit(0, LIMIT)
    assert not host.stplan_past_limit(0, 0) and host.stplan_past_limit(2 ** 32 - 17, 2 ** 32)


def test_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "store_plan_host_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    assert r.stdout.strip() == "%d cases, 0 bad" % (3 * 5 * 3 * 4 * 2 + 32)
