"""k_pileup_fast's deep-tile list (csrc/pileup_schedule_core.h): k_ranges lists the tiles with COVERM_KNOBS pileup_deep_min candidate runs
or more, every wave visits its share of the list first, one tile per visit, and then its chunks without the listed tiles.  The order of
the visits cannot change a result (every output is an integer sum), so for every threshold the integer statistics, the histogram and the
estimator floats must equal, bit for bit, the oracle's and the same session's under COVERM_PILEUP=stream.

The inputs are small, so that a lowered threshold is what makes tiles deep: four contigs of 1 500 - 20 000 bases, one of them ~50 x as deep
as the others, so that its 20 consecutive tiles outnumber the waves of the launch, 10 at the most (list entries w, w + n_waves).  What each input is
named for is checked on the CPU first, in numpy and against the oracle's depth."""
import numpy as np
import pytest

from coverm_amd.engine import FilterConfig, Session
from oracle import oracle as O
from tests.knobs import set_knobs
from tests.test_gpu_abi_parity import _long_read_batch, to_bamdata, to_batch
from tests.test_gpu_hist_derived_stats import FF, STAT_FIELDS, batch_of, bins_of, check_hist, check_stats, estimators, oracle_contig_floats

pytestmark = pytest.mark.gpu

TILE, EXCL, RL = 1024, 75, 100
FAST_MAX_CAND, LDS_BINS, DEFAULT_DEEP_MIN = 8191, 512, 192
CHUNK, CHUNK_LISTED = 4, 8         # tiles per chunk without and with the list (pileup_schedule_core.h); a wave per workgroup, a wave per chunk on a small grid
LENS = np.asarray([20_000, 6_000, 1_500, 9_000], dtype=np.int64)
PILE_AT = 5 * TILE + 200           # 600 identical reads: depth >= 512 in an interior tile of contig 0 (the general loop)
SLOW_TILE = 12                     # 8 300 reads that start and end inside this tile of contig 0: more than FAST_MAX_CAND candidates


def _reads():
    rng = np.random.default_rng(7)
    reads = [(0, int(p), RL) for p in rng.integers(0, LENS[0] - RL + 1, 7000)]
    reads += [(0, int(LENS[0]) - RL, RL)] * 30                   # reads that end at the contig's last base
    reads += [(0, PILE_AT, RL)] * 600
    reads += [(0, int(p), RL) for p in rng.integers(SLOW_TILE * TILE, (SLOW_TILE + 1) * TILE - RL, 8300)]
    for t, n in ((1, 90), (2, 20), (3, 130)):
        reads += [(t, int(p), RL) for p in rng.integers(0, LENS[t] - RL + 1, n)]
    return reads


def tile_candidates(b):
    """(contig, first base, candidate runs) of every tile as k_ranges counts them for position-sorted reads of one length RL: the records
    that start inside the tile and the ones that start up to RL - 1 bases left of it."""
    out = []
    for c, L in enumerate(b.ref_lens):
        pos = b.pos[b.tid == c].astype(np.int64)
        for lo in range(0, int(L), TILE):
            out.append((c, lo, int(((pos > lo - RL) & (pos < lo + TILE)).sum())))
    return np.asarray(out, dtype=np.int64)


_cache = {}


def main_input():
    """(BamData, oracle integer statistics / histogram / primary count, oracle floats, tile candidates): built and evaluated once."""
    if "main" not in _cache:
        b = to_bamdata(batch_of(_reads()), LENS)
        _cache["main"] = (b, O.integer_stats(b, O.FlagFilter(*FF), None, EXCL), oracle_contig_floats(b, estimators(EXCL)[1]), tile_candidates(b))
    return _cache["main"]


def expected_deep(cand, deep_min, mask=None):
    """tiles the list must hold: live, taken by k_pileup_fast (at most FAST_MAX_CAND candidates), deep_min candidates or more"""
    if deep_min == 0:
        return 0
    n = cand[:, 2]
    ok = (n >= max(1, deep_min)) & (n <= FAST_MAX_CAND)
    if mask is not None:
        ok &= np.asarray(mask)[cand[:, 0]] != 0
    return int(ok.sum())


def run(b, mask=None, finishes=1, excl=EXCL):
    """One session with the estimators set: (statistics, histogram, floats, pileup_schedule(), last_paths()) of its last finish and the
    deep-tile counts of all of them."""
    counts = []
    with Session(0, FilterConfig(*FF), excl, want_hist=True, want_identity=True) as s:
        s.set_targets(b.ref_lens, mask)
        if mask is None:       # (a session with a target mask evaluates no estimators on the device: its floats are the host's, from these integers)
            s.set_estimators(estimators(excl)[0])
        s.push(to_batch(b))
        for _ in range(finishes):
            st, summ = s.finish()
            counts.append(s.pileup_schedule()["deep_tiles"])
        ef = s.estimates().copy() if mask is None else np.zeros((len(b.ref_lens), 4), np.float32)
        return dict(st=st.copy(), ef=ef, hist=s.hist().copy(), sched=s.pileup_schedule(), paths=s.last_paths(), counts=counts,
                    prim=int(summ.num_detected_primary_alignments))


def same_results(a, r):
    for f in STAT_FIELDS + ("hist_off",):
        np.testing.assert_array_equal(a["st"][f], r["st"][f], err_msg=f)
    np.testing.assert_array_equal(a["hist"], r["hist"])
    np.testing.assert_array_equal(a["ef"].view(np.uint32), r["ef"].view(np.uint32))
    assert a["prim"] == r["prim"]


def stream_reference(monkeypatch, key, b, **kw):
    """the same session under COVERM_PILEUP=stream (k_pileup_stream over every tile: no list, no flags), once per input"""
    if key not in _cache:
        with monkeypatch.context() as m:
            m.setenv("COVERM_PILEUP", "stream")
            r = run(b, **kw)
        assert r["sched"]["deep_tiles"] == 0 and r["paths"]["slow_tiles"] == 0, r["sched"]
        _cache[key] = r
    return _cache[key]


def check_main(monkeypatch, r, mask=None):
    b, (exp, exp_hist, prim), floats, _ = main_input()
    live = None if mask is None else (exp["seen"] == 1) & (np.asarray(mask) != 0)
    if mask is not None:
        exp, exp_hist, prim = _cache.setdefault(("masked", tuple(mask)), O.integer_stats(b, O.FlagFilter(*FF), None, EXCL, mask))
    assert r["prim"] == prim
    check_stats(r["st"], exp, live)
    check_hist(r["st"], r["hist"], exp, exp_hist, live)
    if mask is None:
        np.testing.assert_array_equal(r["ef"].view(np.uint32), floats.view(np.uint32))
    same_results(r, stream_reference(monkeypatch, ("stream", None if mask is None else tuple(mask)), b, mask=mask))


def test_the_input_holds_the_tiles_it_is_named_for():
    """CPU only (numpy and the oracle): the deep contig is 40 - 100 x as deep as the others and its qualifying tiles are consecutive and
    outnumber the launch's waves; a deep tile lies at the contig's end and one straddles each end of the end-exclusion window; a tile of
    512 or more candidates whose depth reaches 512; a tile of more than FAST_MAX_CAND candidates."""
    b, (exp, _, _), _, cand = main_input()
    depth = [np.cumsum(O.contig_deltas(b, O.FlagFilter(*FF), t, O.reader_stage(b, None)[0]), dtype=np.int64) for t in range(len(LENS))]
    mean = np.asarray([d[:int(L)].mean() for d, L in zip(depth, LENS)])
    assert 40 <= mean[0] / mean[1:].max() and mean[0] / mean[1:].min() <= 100, mean
    c0 = cand[cand[:, 0] == 0]
    n_tiles = len(cand)
    assert n_tiles == 37 and len(c0) == 20
    n_waves = -(-n_tiles // CHUNK)       # a wave per chunk; fewer with the longer chunks of a launch that has the list
    assert n_waves == 10
    for th in (1, 8, 64):       # every tile of the deep contig but the one left to k_pileup_stream
        assert ((c0[:, 2] >= th) & (c0[:, 2] <= FAST_MAX_CAND)).sum() == 19 > n_waves
        assert (cand[cand[:, 0] != 0][:, 2] >= 64).sum() == 0
    deep = (c0[:, 2] >= DEFAULT_DEEP_MIN) & (c0[:, 2] <= FAST_MAX_CAND)
    assert deep.sum() > n_waves and deep[:SLOW_TILE].all()                  # consecutive, more than the waves, at the default too
    assert deep[0] and 0 < EXCL < TILE                                      # a deep tile straddles the window's start
    last = c0[-1]
    assert last[1] < LENS[0] - EXCL < LENS[0] < last[1] + TILE and last[2] >= 64     # the contig's last tile holds the window's end and the contig's
    pile_tile = PILE_AT // TILE
    assert LDS_BINS <= c0[pile_tile, 2] <= FAST_MAX_CAND and depth[0][PILE_AT:PILE_AT + RL].min() >= LDS_BINS
    assert EXCL <= pile_tile * TILE and (pile_tile + 1) * TILE <= LENS[0] - EXCL     # interior: only the candidate count sends it to the general loop
    assert c0[SLOW_TILE, 2] > FAST_MAX_CAND and (np.delete(cand[:, 2], SLOW_TILE) <= FAST_MAX_CAND).all()
    assert exp["win_max_d"][0] >= LDS_BINS


@pytest.mark.parametrize("deep_min", [0, 1, 8, 64, None], ids=lambda v: "default" if v is None else "min%d" % v)
def test_every_threshold_gives_the_oracles_and_the_stream_kernels_results(deep_min, monkeypatch):
    b, _, _, cand = main_input()
    if deep_min is not None:
        set_knobs(monkeypatch, pileup_deep_min=deep_min)
    r = run(b)
    th = DEFAULT_DEEP_MIN if deep_min is None else deep_min
    chunk = CHUNK_LISTED if th else CHUNK
    assert r["sched"]["deep_min"] == th and r["sched"]["chunk_tiles"] == chunk and r["sched"]["waves"] == -(-len(cand) // chunk), r["sched"]
    want = expected_deep(cand, th)
    assert (want > 0) == (th > 0) and r["sched"]["deep_tiles"] == want, (r["sched"], want)
    assert r["paths"]["slow_tiles"] == 1, r["paths"]         # the tile beyond FAST_MAX_CAND: on the slow list, so never on the deep list (want excludes it)
    check_main(monkeypatch, r)


@pytest.mark.parametrize("chunk_tiles", [1, 4, 7])
def test_chunk_sizes(chunk_tiles, monkeypatch):
    b, _, _, cand = main_input()
    set_knobs(monkeypatch, pileup_deep_min=8, pileup_chunk_tiles=chunk_tiles)
    r = run(b)
    n_chunks = -(-len(cand) // chunk_tiles)
    assert r["sched"]["chunk_tiles"] == chunk_tiles and r["sched"]["waves"] == n_chunks, r["sched"]
    assert r["sched"]["deep_tiles"] == expected_deep(cand, 8) > 0
    check_main(monkeypatch, r)


def test_the_two_table_kernel_takes_the_list_too(monkeypatch):
    b, _, _, cand = main_input()
    set_knobs(monkeypatch, pileup_deep_min=8)
    monkeypatch.setenv("COVERM_FAST_TABLES", "2")
    r = run(b)
    assert r["sched"]["deep_tiles"] == expected_deep(cand, 8) > 0
    check_main(monkeypatch, r)


@pytest.mark.parametrize("deep_min", [1, None], ids=["min1", "default"])
def test_a_target_mask_that_removes_the_deep_contig(deep_min, monkeypatch):
    """The masked contig's tiles have no candidates: at the default nothing is left to list, at 1 the other contigs' covered tiles are."""
    b, _, _, cand = main_input()
    mask = np.asarray([0, 1, 1, 1], dtype=np.uint8)
    if deep_min is not None:
        set_knobs(monkeypatch, pileup_deep_min=deep_min)
    r = run(b, mask=mask)
    want = expected_deep(cand, DEFAULT_DEEP_MIN if deep_min is None else deep_min, mask)
    assert (want > 0) == (deep_min == 1) and r["sched"]["deep_tiles"] == want, (r["sched"], want)
    assert r["paths"]["slow_tiles"] == 0, r["paths"]
    check_main(monkeypatch, r, mask=mask)


def test_a_second_finish_lists_the_same_tiles(monkeypatch):
    """k_init zeroes the list's counter in front of every pass: a finish repeated on one session lists as many tiles as the first."""
    b, _, _, cand = main_input()
    set_knobs(monkeypatch, pileup_deep_min=8)
    r = run(b, finishes=3)
    assert r["counts"] == [expected_deep(cand, 8)] * 3 and r["counts"][0] > 0, r["counts"]
    check_main(monkeypatch, r)


def test_a_long_cigar_sample_whose_pass_is_repeated(monkeypatch):
    """Long reads whose bucket entries do not fit the first buffer: the pipeline runs twice over the store, the second pass's k_ranges
    lists the tiles again from a zeroed counter, and the tiles' bucket entries count towards the threshold."""
    ref_lens = np.asarray([20_000, 9_000, 4_000], dtype=np.int64)
    batch = _long_read_batch(ref_lens, 400, 1_500, seed=31)
    nops = np.diff(batch.cigar_off.astype(np.int64))
    assert (nops > 16).sum() > 50          # records that go through the per-tile buckets (CX_MIN_OPS)
    b = to_bamdata(batch, ref_lens)
    exp, exp_hist, prim = O.integer_stats(b, O.FlagFilter(*FF), None, EXCL)
    floats = oracle_contig_floats(b, estimators(EXCL)[1])
    with monkeypatch.context() as m:
        m.setenv("COVERM_PILEUP", "stream")
        ref = run(b)
    for deep_min in (0, 8):
        with monkeypatch.context() as m:
            set_knobs(m, pileup_deep_min=deep_min)
            r = run(b)
        assert r["paths"]["passes"] == 2 and r["paths"]["bucket_entries"] > 0, r["paths"]
        assert (r["sched"]["deep_tiles"] > 0) == (deep_min > 0) and r["sched"]["deep_tiles"] <= 33, r["sched"]
        assert r["prim"] == prim
        check_stats(r["st"], exp)
        check_hist(r["st"], r["hist"], exp, exp_hist)
        np.testing.assert_array_equal(r["ef"].view(np.uint32), floats.view(np.uint32))
        same_results(r, ref)
