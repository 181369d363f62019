"""--unsorted on the host: covh_group_by_reference (the stable counting sort the whole-file paths use ahead of the host's pair filter and the
gene driver) against numpy's stable argsort of the same keys, and the refusals the argument parser gives before any device is touched."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from coverm_amd import native
from tests import binary
from tests.grouping import grouped_order


def host_order(tid, n_targets):
    L = native.lib()
    L.covh_group_by_reference.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.c_uint64)]
    L.covh_free.argtypes = [C.c_void_p]
    L.covh_free.restype = None
    tid = np.ascontiguousarray(tid, np.int32)
    p, moved = C.POINTER(C.c_uint64)(), C.c_uint64(0)
    assert L.covh_group_by_reference(tid.ctypes.data if len(tid) else None, len(tid), n_targets, C.byref(p), C.byref(moved)) == 0
    out = np.ctypeslib.as_array(p, shape=(max(len(tid), 1),))[:len(tid)].copy()
    L.covh_free(p)
    return out, int(moved.value)


@pytest.mark.parametrize("n_targets", [1, 255, 256, 257, 65_536, 2_000_000])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4095, 4096, 4097, 300_000])
def test_matches_numpy_stable_order(n, n_targets):
    rng = np.random.default_rng(n + n_targets)
    tid = rng.integers(-1, n_targets, n).astype(np.int32)
    want = grouped_order(tid, n_targets)
    got, moved = host_order(tid, n_targets)
    np.testing.assert_array_equal(got, want.astype(np.uint64))
    assert moved == int((want != np.arange(n)).sum())


def test_special_inputs():
    for tid, nt in [(np.full(5000, 3), 9), (np.arange(5000)[::-1], 5000), (np.where(np.arange(7000) % 3 == 0, -1, 0), 2_000_000), (np.full(100, -1), 4),
                    (np.asarray([2, 9, 1, -7, 1]), 3)]:      # (a tid at or beyond n_targets shares the key of the records without a reference)
        want = grouped_order(tid, nt)
        got, moved = host_order(tid, nt)
        np.testing.assert_array_equal(got, want.astype(np.uint64))
        assert moved == int((want != np.arange(len(tid))).sum())
    tid = np.sort(np.random.default_rng(2).integers(0, 500, 100_000)).astype(np.int32)
    tid[-100:] = -1
    got, moved = host_order(tid, 500)
    assert moved == 0 and (got == np.arange(len(tid))).all()


def _stderr_of(argv):
    r = subprocess.run(argv, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and r.stdout == ""
    return r.stderr


def test_filter_refuses_the_flag(tmp_path):
    err = _stderr_of([binary.BIN, "filter", "-b", str(tmp_path / "in.bam"), "-o", str(tmp_path / "out.bam"), "--unsorted"])
    assert "--unsorted" in err and "filter" in err
    assert not (tmp_path / "out.bam").exists()


def test_span_mode_refuses_the_flag(tmp_path):
    """Fewer files than devices: a file would be cut into tid spans.  Refused while the arguments are read — the files are never opened."""
    for mode in ("contig", "genome"):
        err = _stderr_of([binary.BIN, mode, "-b", str(tmp_path / "a.bam"), "--unsorted", "--devices", "0,1"] + (["-s", "~"] if mode == "genome" else []))
        assert "--unsorted" in err and "--devices" in err and "fewer" in err
