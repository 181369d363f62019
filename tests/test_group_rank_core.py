"""csrc/group_rank_core.h (the rank arithmetic of cov_group_records' radix sort: digit of a key, peers mask from the wave's ballots, rank
among the peers, the waves' bases, the digit-major histogram) run on the CPU: tests/c/group_rank_host.cpp loops over workgroups, waves and
lanes exactly as k_group_hist / k_group_scatter lay them out; the permutation of every case must be numpy's stable argsort of the keys."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("grpk") / "grpk_host.so")
    subprocess.check_call(["g++", "-O2", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "c", "group_rank_host.cpp")])
    L = C.CDLL(so)
    L.grpk_host_order.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_int]
    L.grpk_host_order.restype = C.c_uint32
    L.grpk_host_passes.argtypes = [C.c_uint32]
    L.grpk_host_passes.restype = C.c_uint32
    L.grpk_host_key.argtypes = [C.c_int32, C.c_uint32]
    L.grpk_host_key.restype = C.c_uint32
    return L


def keys_of(tid, n_targets):
    """rec_key's order: a reference's tid, n_targets for a record without one."""
    t = np.asarray(tid, np.int64)
    return np.where((t >= 0) & (t < n_targets), t, n_targets)


def order_of(L, tid, n_targets, reverse=0):
    tid = np.ascontiguousarray(tid, np.int32)
    out = np.full(len(tid), 0xFFFFFFFF, np.uint32)
    passes = L.grpk_host_order(tid.ctypes.data if len(tid) else None, len(tid), n_targets, out.ctypes.data if len(tid) else None, reverse)
    return out, passes


def check(L, tid, n_targets):
    want = np.argsort(keys_of(tid, n_targets), kind="stable").astype(np.uint32)
    for reverse in (0, 1):
        got, passes = order_of(L, tid, n_targets, reverse)
        np.testing.assert_array_equal(got, want)
        assert passes == L.grpk_host_passes(n_targets)


SIZES = [0, 1, 63, 64, 65, 4095, 4096, 4097, 300_000]
TARGETS = [1, 255, 256, 257, 65_536, 2_000_000]


def test_passes_and_keys(host):
    """Digits of 8 bits, as many as the keys 0 .. n_targets need: ceil(log2(n_targets + 1)) / 8, rounded up."""
    for nt, p in [(1, 1), (2, 1), (255, 1), (256, 2), (257, 2), (5000, 2), (65_535, 2), (65_536, 3), (200_000, 3), (2_000_000, 3), (1 << 24, 4), (0xFFFFFFF0, 4)]:
        assert host.grpk_host_passes(nt) == p, nt
        assert p == max(1, -(-int(nt).bit_length() // 8))
    assert host.grpk_host_key(0, 7) == 0 and host.grpk_host_key(6, 7) == 6
    assert host.grpk_host_key(-1, 7) == 7 and host.grpk_host_key(-5, 7) == 7 and host.grpk_host_key(7, 7) == 7


@pytest.mark.parametrize("n_targets", TARGETS)
@pytest.mark.parametrize("n", SIZES)
def test_random_keys(host, n, n_targets):
    rng = np.random.default_rng(n * 31 + n_targets)
    tid = rng.integers(-1, n_targets, n).astype(np.int32)
    check(host, tid, n_targets)


@pytest.mark.parametrize("n", SIZES)
def test_one_key(host, n):
    for nt, v in [(1, 0), (257, 256), (2_000_000, 1_234_567), (300, -1)]:
        check(host, np.full(n, v, np.int32), nt)


@pytest.mark.parametrize("n", SIZES)
def test_distinct_descending(host, n):
    nt = max(n, 1)
    check(host, np.arange(n, dtype=np.int32)[::-1].copy(), nt)
    check(host, np.arange(n, dtype=np.int32)[::-1].copy(), 2_000_000)


@pytest.mark.parametrize("n_targets", TARGETS)
@pytest.mark.parametrize("n", SIZES)
def test_only_zero_and_unmapped(host, n, n_targets):
    """Keys 0 and n_targets only: every digit of the top key takes part, and nothing else does."""
    rng = np.random.default_rng(n + 7)
    tid = np.where(rng.integers(0, 2, n) == 1, 0, -1).astype(np.int32)
    check(host, tid, n_targets)


@pytest.mark.parametrize("n_targets", TARGETS)
@pytest.mark.parametrize("n", SIZES)
def test_grouped_input_is_the_identity(host, n, n_targets):
    rng = np.random.default_rng(n + 11)
    tid = np.sort(keys_of(rng.integers(-1, n_targets, n), n_targets)).astype(np.int64)
    tid = np.where(tid == n_targets, -1, tid).astype(np.int32)
    got, _ = order_of(host, tid, n_targets)
    np.testing.assert_array_equal(got, np.arange(n, dtype=np.uint32))


def test_tile_and_wave_boundaries(host):
    """Runs of one key that straddle a wave (64), a round (256) and a tile (4096), between runs of other keys."""
    for cut in (64, 256, 4096):
        for d in (-1, 0, 1):
            n = 3 * 4096 + 17
            tid = np.full(n, 5, np.int32)
            tid[cut + d:cut + d + 300] = 3
            tid[::7] = 9
            tid[5::64] = -1
            check(host, tid, 300)
