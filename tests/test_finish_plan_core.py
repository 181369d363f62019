"""csrc/finish_plan_core.h (the decisions of one pass of the device pipeline: which kernels run, on which stream, and the sizes of their
launches, taken once from the session's facts) against the same decisions as finish_once took them while each stood where the pass first
needed it, frozen in tests/c/finish_plan_host.cpp, over a grid that straddles every threshold; and against a few of them written out here.
The program form of the same file walks the same grid built with -fsanitize=address,undefined."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "c", "finish_plan_host.cpp")
FIELDS = ("long_cigars", "prep_passes", "prep_chunk", "prep_grid", "n_steps", "gen_all", "gen_grid", "est_lanes", "run_prep", "prep7", "run_pileup",
          "identity_side", "id_primary", "id_nonsupp", "compacted", "derive_in_est", "hist_stats_launch", "hist_prefetch", "nf", "runs", "genomes",
          "genome_identity", "lean_error", "ncig", "want_hist", "want_id", "lean", "genome_lanes_from")
NUMBERS = ("prep_passes", "prep_chunk", "prep_grid", "n_steps", "gen_grid", "nf", "ncig", "genome_lanes_from")
BOOLS = tuple(f for f in FIELDS if f not in NUMBERS)
# R x nT x tiles x CIGAR words x est.n x knob x prep kernel x CUs x want bits x boolean facts
CASES = 11 * 5 * 3 * 3 * 2 * 3 * 2 * 2 * 16 * 128
HIST, IDENT, PRIMARY_ONLY, NONSUPP_ONLY = 1, 2, 4, 8
MASK, RUNS, GENOMES, SPILL, IN_SPILL, LEAN, FETCH_SEEN = (1 << k for k in range(7))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("finplan") / "finish_plan_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-o", so, SRC])
    L = C.CDLL(so)
    assert L.finplan_n_fields() == len(FIELDS)
    for f in (L.finplan_plan, L.finplan_frozen):
        f.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_void_p]
        f.restype = None
    L.finplan_walk.argtypes = [C.c_void_p, C.c_void_p]
    L.finplan_walk.restype = C.c_uint64
    return L


def plan(host, R=12800, nT=3, n_tiles=100, ncig=None, want=HIST, est_n=1, knob=-1, prep_kernel=0, n_cus=256, flags=0, fn="finplan_plan"):
    out = np.zeros(len(FIELDS), np.uint64)
    getattr(host, fn)(R, nT, n_tiles, R if ncig is None else ncig, want, est_n, knob, prep_kernel, n_cus, flags, out.ctypes.data)
    return dict(zip(FIELDS, (int(x) for x in out)))


@pytest.fixture(scope="module")
def walked(host):
    bad = C.c_uint64(0)
    seen = np.zeros((2, len(FIELDS)), np.uint64)
    n = host.finplan_walk(C.byref(bad), seen.ctypes.data)
    return n, bad.value, seen


def test_plan_equals_the_frozen_decisions_on_the_grid(walked):
    n, bad, _ = walked
    assert n == CASES
    assert bad == 0


def test_every_boolean_takes_both_values_and_the_error_occurs(walked):
    _, _, seen = walked
    for k, f in enumerate(FIELDS):
        assert seen[1][k], f
        if f in BOOLS:
            assert seen[0][k], f
    assert seen[1][FIELDS.index("lean_error")] and seen[0][FIELDS.index("lean_error")]


def test_thresholds_written_out(host):
    """The thresholds the grid straddles, one by one, against numbers worked out by hand."""
    assert plan(host, R=4096)["prep_grid"] == 1 and plan(host, R=4097)["prep_grid"] == 2 and plan(host, R=0)["prep_grid"] == 0
    assert plan(host, R=100, ncig=1599)["long_cigars"] == 0 and plan(host, R=100, ncig=1600)["long_cigars"] == 1
    assert plan(host, R=100, ncig=1600)["prep_chunk"] == 256 and plan(host, R=100, ncig=1599)["prep_chunk"] == 4096
    assert plan(host, R=1279, nT=10)["gen_all"] == 1 and plan(host, R=1280, nT=10)["gen_all"] == 0
    assert plan(host, R=1279, nT=10, prep_kernel=7)["gen_all"] == 0 and plan(host, R=1279, nT=10, prep_kernel=7)["prep7"] == 1
    assert plan(host, R=64)["n_steps"] == 1 and plan(host, R=65)["n_steps"] == 2
    assert plan(host, R=12800, nT=1, n_cus=1)["gen_grid"] == 8 and plan(host, R=12800, nT=1000, n_cus=1)["gen_grid"] == 50      # 200 steps: 8 x CUs, or 64 x CUs and (200 + 3) / 4
    assert plan(host, nT=65535)["est_lanes"] == 0 and plan(host, nT=65536)["est_lanes"] == 1
    assert plan(host, nT=65536, knob=0)["est_lanes"] == 0 and plan(host, nT=1, knob=1)["est_lanes"] == 1
    # a lane per genome: from 65 536 entries on whatever the contigs' count (nG >= genome_lanes_from), the knob forces it on / off
    assert plan(host, nT=1)["genome_lanes_from"] == 65536 and plan(host, nT=65536)["genome_lanes_from"] == 65536
    assert plan(host, nT=65536, knob=1)["genome_lanes_from"] == 0 and plan(host, nT=65536, knob=0)["genome_lanes_from"] == 0xffffffff
    assert plan(host, nT=3, est_n=1)["nf"] == 3 and plan(host, nT=3, est_n=1, flags=MASK)["nf"] == 0 and plan(host, nT=3, est_n=1, flags=RUNS)["nf"] == 0


def test_histogram_decisions(host):
    p = plan(host)                                   # histogram and estimators: the estimator kernel derives, nothing is compacted
    assert (p["compacted"], p["derive_in_est"], p["hist_stats_launch"], p["hist_prefetch"]) == (0, 1, 0, 0)
    p = plan(host, flags=FETCH_SEEN)                 # the caller fetched the last histogram: compacted and prefetched, k_hist_stats derives
    assert (p["compacted"], p["derive_in_est"], p["hist_stats_launch"], p["hist_prefetch"]) == (1, 0, 1, 1)
    p = plan(host, est_n=0)                          # no estimators
    assert (p["compacted"], p["derive_in_est"], p["hist_stats_launch"], p["hist_prefetch"]) == (1, 0, 1, 0)
    p = plan(host, flags=MASK)                       # a target mask: no per-contig estimator kernel to derive anything
    assert (p["compacted"], p["derive_in_est"], p["hist_stats_launch"]) == (0, 0, 1)
    for nothing in (dict(R=0), dict(n_tiles=0)):     # nothing is piled up: nothing compacted, derived or prefetched, whatever was fetched
        p = plan(host, flags=FETCH_SEEN, **nothing)
        assert (p["run_pileup"], p["compacted"], p["derive_in_est"], p["hist_stats_launch"], p["hist_prefetch"]) == (0, 0, 0, 0, 0)
    p = plan(host, want=0)
    assert (p["compacted"], p["derive_in_est"], p["hist_stats_launch"]) == (0, 0, 0)


def test_identity_and_genome_decisions(host):
    p = plan(host, want=HIST | IDENT)
    assert (p["identity_side"], p["id_primary"], p["id_nonsupp"]) == (1, 1, 1)
    assert plan(host, want=IDENT | PRIMARY_ONLY)["id_nonsupp"] == 0 and plan(host, want=IDENT | NONSUPP_ONLY)["id_primary"] == 0
    assert plan(host, want=IDENT, R=0)["identity_side"] == 0 and plan(host, want=IDENT, nT=0)["identity_side"] == 0
    assert plan(host, want=PRIMARY_ONLY)["id_primary"] == 0          # the bits mean nothing without COV_WANT_IDENTITY
    assert plan(host, flags=GENOMES | MASK)["genomes"] == 1 and plan(host, flags=GENOMES | MASK)["runs"] == 0
    assert plan(host, flags=RUNS)["runs"] == 1 and plan(host, flags=RUNS)["genomes"] == 1
    for off in (SPILL, IN_SPILL):
        assert plan(host, flags=RUNS | off)["genomes"] == 0 and plan(host, flags=GENOMES | MASK | off)["genomes"] == 0
    assert plan(host, flags=RUNS, est_n=0)["genomes"] == 0
    assert plan(host, flags=LEAN)["lean_error"] == 1 and plan(host, flags=LEAN | RUNS)["lean_error"] == 0 and plan(host, flags=LEAN | RUNS | SPILL)["lean_error"] == 1
    assert plan(host, want=IDENT | PRIMARY_ONLY, flags=GENOMES | MASK)["genome_identity"] == 0 and plan(host, want=IDENT | PRIMARY_ONLY, flags=RUNS)["genome_identity"] == 1
    assert plan(host, want=IDENT | NONSUPP_ONLY, flags=RUNS)["genome_identity"] == 0


def test_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "finish_plan_host_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror", "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    assert r.stdout.strip() == "%d cases, 0 bad" % CASES
