"""With the histogram wanted the pileup kernels produce a contig's depth histogram and one counter (covered positions outside the window);
the window statistics — sum d, sum d^2, covered, min, max, window positions seen — are derived from the final bins once per contig
(csrc/hist_stats_core.h): as the prologue of k_estimate / k_estimate_lanes when the estimator kernel is the first reader, by a k_hist_stats
launch behind the pileup otherwise.  Every integer statistic and every histogram bin against the CPU oracle, bit for bit, on inputs built
around what could go wrong: windows of no and of one base, tiles no read touches, depths on both sides of the 512 LDS bins, contig changes
inside a wave's chunk of tiles, a tile that goes to k_pileup_stream beside tiles of k_pileup_fast, every consumer that reads the derived
fields in front of the estimator kernel, and an assembly (a lane per contig).  Tiles are 1024 bases; a wave walks chunks of 4 consecutive tiles (8 until this change)."""
import numpy as np
import pytest

from coverm_amd.engine import FilterConfig, RecordBatch, Session
from coverm_amd.host import CoverageEstimator as E
from coverm_amd.native import CovError
from oracle import oracle as O
from tests.knobs import set_knobs
from tests.test_gpu_abi_parity import compare, to_bamdata, to_batch

pytestmark = pytest.mark.gpu

FF = (True, True, False)
TILE = 1024
STAT_FIELDS = ("n_primary", "n_pass", "n_nonsupp", "sum_nm", "sum_indel", "win_sum_d", "win_sum_d2", "win_covered", "full_covered", "win_min_d",
               "win_max_d", "hist_len")


# ------------------------------------------------------------------ inputs
def batch_of(reads):
    """reads: (tid, pos, length) of plain `M` alignments, any order."""
    r = np.asarray(sorted(reads), dtype=np.int64).reshape(-1, 3)
    n = len(r)
    return RecordBatch.from_arrays(r[:, 0], r[:, 1], np.full(n, 99), np.full(n, 30), np.ones(n), np.ones(n), r[:, 2],
                                   np.arange(n + 1, dtype=np.uint32), ((r[:, 2] << 4) | 0).astype(np.uint32))


def sprinkle(rng, tid, lo, hi, n, max_len=150):
    """n reads inside [lo, hi) of contig tid."""
    out = []
    for _ in range(n):
        ln = int(rng.integers(1, min(max_len, hi - lo) + 1))
        out.append((tid, int(rng.integers(lo, hi - ln + 1)), ln))
    return out


def input_windows(excl):
    """Contigs no longer than 2 x excl (no window), of 2 x excl + 1 (a window of one base), of one tile and one base, and around them."""
    lens = [max(1, 2 * excl - 50), max(1, 2 * excl), 2 * excl + 1, 2 * excl + 2, TILE + 1, TILE, 2 * TILE + 1, 3000]
    rng = np.random.default_rng(100 + excl)
    reads = []
    for t, L in enumerate(lens):
        reads += sprinkle(rng, t, 0, L, 40)
        reads += [(t, 0, L), (t, L - 1, 1), (t, 0, 1)]          # end to end, the last base, the first base
    return lens, batch_of(reads)


def input_untouched_tile(excl):
    """Five tiles, reads in tiles 0, 1 and 4 only: the window positions of tiles 2 and 3 are in no bin."""
    lens = [5 * TILE - 100, 700]
    rng = np.random.default_rng(7)
    reads = sprinkle(rng, 0, 0, 2 * TILE, 300) + sprinkle(rng, 0, 4 * TILE, lens[0], 200) + sprinkle(rng, 1, 0, 700, 30)
    reads += [(0, 100, 2 * TILE - 100)]          # every window position of tiles 0 and 1 covered: the depth-0 bin comes from the gap alone
    return lens, batch_of(reads)


def input_bins(last_tile):
    """Columns of depth 511, 512 and 513 — the LDS bins hold depths below 512, and a tile with fewer than 512 candidate runs never leaves
    them — one contig each, alone in their tile, and the three depths side by side in a fourth contig; on an interior tile of a five-tile
    contig, or on its (partial) last tile."""
    def make(excl):
        L = 4 * TILE + 600
        lo = 4 * TILE + 100 if last_tile else 2 * TILE + 100
        lens = [L, L, L, L]
        rng = np.random.default_rng(511)
        reads = []
        for t, depth in enumerate((511, 512, 513)):
            reads += [(t, lo, 200)] * depth + sprinkle(rng, t, 0, 2 * TILE, 60)
        reads += [(3, lo, 300)] * 511 + [(3, lo + 100, 200)] + [(3, lo + 200, 100)] + sprinkle(rng, 3, 0, 2 * TILE, 60)
        return lens, batch_of(reads)
    return make


def input_borders(excl):
    """A contig of 20 tiles (five chunks of 4, the default; more than two of 8) and two of 3 tiles behind it (a contig change inside a
    chunk at either size; test_chunk_sizes_by_the_knob runs it at 1, 3 and 8 too); reads in every tile."""
    lens = [20 * TILE - 37, 3 * TILE - 500, 3 * TILE]
    rng = np.random.default_rng(20)
    reads = []
    for t, L in enumerate(lens):
        for lo in range(0, L, TILE):
            reads += sprinkle(rng, t, lo, min(lo + TILE, L), 25)
        reads += sprinkle(rng, t, 0, L, 60, max_len=2500)          # and reads across tile borders
    return lens, batch_of(reads)


INPUTS = {"windows": input_windows, "untouched_tile": input_untouched_tile, "bins_interior": input_bins(False), "bins_last": input_bins(True),
          "borders": input_borders}
_cache = {}


def sample(name, excl):
    """(BamData, the oracle's (stats, hist, primary count)) of one input: built and evaluated once, shared by every test that needs it."""
    key = (name, excl)
    if key not in _cache:
        lens, batch = INPUTS[name](excl)
        b = to_bamdata(batch, np.asarray(lens, np.int64))
        _cache[key] = (b, O.integer_stats(b, O.FlagFilter(*FF), None, excl))
    return _cache[key]


# ------------------------------------------------------------------ checks
def bins_of(hist, off, n):
    """the bins of every contig behind each other (hist[off[t] : off[t] + n[t]] for every t), without a loop over contigs"""
    n = n.astype(np.int64)
    start = np.repeat(off.astype(np.int64) - np.concatenate(([0], np.cumsum(n)[:-1])), n)
    return hist[start + np.arange(int(n.sum()))]


def check_stats(st, exp, live=None, fields=STAT_FIELDS):
    live = (exp["seen"] == 1) if live is None else live
    for f in fields:
        np.testing.assert_array_equal(st[f][live], exp[f][live], err_msg=f)
        if f not in ("n_primary", "n_pass", "n_nonsupp"):
            assert (st[f][~live] == 0).all(), f


def check_hist(st, hist, exp, exp_hist, live=None):
    live = (exp["seen"] == 1) if live is None else live
    np.testing.assert_array_equal(st["hist_len"][live], exp["hist_len"][live])
    assert (st["hist_len"][~live] == 0).all()
    np.testing.assert_array_equal(bins_of(hist, st["hist_off"][live], st["hist_len"][live]), bins_of(exp_hist, exp["hist_off"][live], exp["hist_len"][live]))


def estimators(excl, want_hist=True):
    """(the session's, the oracle's) — with the histogram: what reads every derived field (sums, covered, min through the variance, the bins
    through the trimmed mean, the full-length covered count); without: the mean alone, which does not want it."""
    if not want_hist:
        return [E.new_estimator_mean(0.0, excl, False)], [O.est_mean(0.0, excl, False)]
    return ([E.new_estimator_mean(0.0, excl, False), E.new_estimator_trimmed_mean(0.05, 0.95, 0.0, excl), E.new_estimator_variance(0.0, excl),
             E.new_estimator_covered_fraction(0.0)],
            [O.est_mean(0.0, excl, False), O.est_trimmed_mean(0.05, 0.95, 0.0, excl), O.est_variance(0.0, excl), O.est_covered_fraction(0.0)])


def oracle_contig_floats(b, est_o):
    taker = O.CachedTaker(len(est_o))
    O.contig_coverage([b], ["s"], taker, est_o, True, O.FlagFilter(*FF))
    rows = np.zeros((len(b.ref_lens), len(est_o)), np.float32)
    filled = np.zeros(len(b.ref_lens), np.int64)
    for entry, cov in taker.coverages[0]:
        rows[entry, filled[entry]] = cov
        filled[entry] += 1
    assert (filled == len(est_o)).all()
    return rows


def estimator_path(b, oracle, excl, want_hist=True):
    """A session with estimators set: the estimator kernel runs right behind the pileup and (with the histogram) derives the statistics as
    its prologue.  Statistics, floats and — fetched after the finish, so compacted from the fields the prologue wrote — the histogram."""
    exp, exp_hist, prim = oracle
    est_e, est_o = estimators(excl, want_hist)
    with Session(0, FilterConfig(*FF), excl, want_hist=want_hist, want_identity=True) as s:
        s.set_targets(b.ref_lens)
        s.set_estimators(est_e)
        s.push(to_batch(b))
        st, summ = s.finish()
        ef = s.estimates()
        assert summ.num_detected_primary_alignments == prim
        check_stats(st, exp, fields=STAT_FIELDS if want_hist else STAT_FIELDS[:-1])
        if want_hist:
            check_hist(st, s.hist(), exp, exp_hist)
    np.testing.assert_array_equal(ef.view(np.uint32), oracle_contig_floats(b, est_o).view(np.uint32))
    return st


def both_paths(name, excl):
    b, oracle = sample(name, excl)
    st = compare(b, ff=FF, excl=excl)          # no estimators: the finish compacts the histogram, k_hist_stats runs behind the pileup
    estimator_path(b, oracle, excl)
    return st, oracle[0]


# ------------------------------------------------------------------ cases 1 - 4
@pytest.mark.parametrize("excl", [0, 75])
def test_windows(excl):
    st, exp = both_paths("windows", excl)
    if excl:
        # no window: every window statistic zero (the device's min_d stays 0xffffffff, which the ABI reports as 0), the full-length count not
        for f in ("win_sum_d", "win_sum_d2", "win_covered", "win_min_d", "win_max_d", "hist_len"):
            assert (st[f][:2] == 0).all(), f
        assert (st["full_covered"][:2] == (2 * excl - 50, 2 * excl)).all()
        assert st["win_covered"][2] == 1          # the window of one base


@pytest.mark.parametrize("excl", [0, 75])
def test_untouched_tile_inside_a_contig(excl):
    st, exp = both_paths("untouched_tile", excl)
    # tiles 0 and 1 are covered end to end: the lowest depth, 0, is seen in the two tiles no read touches (and right of the reads of tile 4) only
    assert st["win_min_d"][0] == 0 and st["win_covered"][0] <= 3 * TILE - 100 - 2 * excl


@pytest.mark.parametrize("excl", [0, 75])
@pytest.mark.parametrize("where", ["bins_interior", "bins_last"])
def test_lds_bin_boundary(where, excl):
    st, exp = both_paths(where, excl)
    assert (st["win_max_d"] == (511, 512, 513, 513)).all()


@pytest.mark.parametrize("excl", [0, 75])
def test_chunk_and_contig_borders(excl):
    both_paths("borders", excl)


@pytest.mark.parametrize("excl", [0, 75])
@pytest.mark.parametrize("chunk", [1, 3, 8])
def test_chunk_sizes_by_the_knob(chunk, excl, monkeypatch):
    """COVERM_KNOBS pileup_chunk_tiles (the default is 4): a chunk per tile, chunks that never end on a contig's border (3 tiles: the
    contigs are 20, 3 and 3 tiles), and the former default of 8 — a wave's tile sequence and every chunk end and contig change inside it
    move, the results do not.  k_pileup_fast, and k_pileup_stream over every tile."""
    set_knobs(monkeypatch, pileup_chunk_tiles=chunk)
    both_paths("borders", excl)
    monkeypatch.setenv("COVERM_PILEUP", "stream")
    both_paths("borders", excl)


# ------------------------------------------------------------------ case 5
def test_slow_tile_beside_fast_tiles():
    """Tile 2 holds 8 192 candidate runs (more than k_pileup_fast's tables take: k_pileup_stream walks it), its neighbours a few dozen:
    one histogram per contig fed by both kernels, depths far beyond the LDS bins."""
    lens = [6 * TILE + 11, 2000]
    rng = np.random.default_rng(5)
    reads = [(0, int(p), 40) for p in rng.integers(2 * TILE, 3 * TILE - 40, 8192)]
    for lo in (0, TILE, 3 * TILE, 4 * TILE, 5 * TILE):
        reads += sprinkle(rng, 0, lo, lo + TILE, 30)
    reads += sprinkle(rng, 1, 0, 2000, 50)
    b = to_bamdata(batch_of(reads), np.asarray(lens, np.int64))
    for excl in (0, 75):
        paths = {}
        compare(b, ff=FF, excl=excl, paths_out=paths)
        assert paths["slow_tiles"] == 1
        estimator_path(b, O.integer_stats(b, O.FlagFilter(*FF), None, excl), excl)


# ------------------------------------------------------------------ case 6
@pytest.mark.parametrize("excl", [0, 75])
@pytest.mark.parametrize("name", list(INPUTS))
@pytest.mark.parametrize("impl", ["stream", "tables2"])
def test_other_implementations(impl, name, excl, monkeypatch):
    if impl == "stream":
        monkeypatch.setenv("COVERM_PILEUP", "stream")
    else:
        monkeypatch.setenv("COVERM_FAST_TABLES", "2")
    both_paths(name, excl)


# ------------------------------------------------------------------ case 7
@pytest.mark.parametrize("excl", [0, 75])
@pytest.mark.parametrize("name", list(INPUTS))
def test_no_histogram(name, excl):
    """A session whose estimators do not want the histogram: the kernels' explicit sums, as before."""
    b, oracle = sample(name, excl)
    estimator_path(b, oracle, excl, want_hist=False)
    with Session(0, FilterConfig(*FF), excl, want_hist=False) as s:          # and without estimators
        s.set_targets(b.ref_lens)
        s.push(to_batch(b))
        st, _ = s.finish()
        check_stats(st, oracle[0], fields=STAT_FIELDS[:-1])


# ------------------------------------------------------------------ case 8
def test_second_finish_compacts_the_histogram():
    """finish, fetch the histogram, finish again: the second finish compacts the histogram itself, so max_d is needed in front of
    k_hist_off<1> — k_hist_stats derives it, not the estimator kernel.  The same statistics, bins and floats from both.
    Then what travels from one pass of the session to the next (the fetch seen, the compaction done, the prefetched bins and their count):
    a third finish behind the second one's fetch compacts and prefetches again and nobody fetches; the fourth, with no fetch since the
    third, goes back to deriving in the estimator's prologue, and the fetch behind it compacts late — nothing of the third's unread
    prefetch may be served; a reset and a finish over no records: rows of zeros, no bins, nothing left over."""
    excl = 75
    b, (exp, exp_hist, prim) = sample("borders", excl)
    est_e, est_o = estimators(excl)
    compactions = []          # launches of the compaction group inside each finish
    with Session(0, FilterConfig(*FF), excl, want_hist=True, want_identity=True) as s:
        s.set_targets(b.ref_lens)
        s.set_estimators(est_e)
        s.push(to_batch(b))
        st1, _ = s.finish()
        compactions.append(s.kernel_ms()["k_hist_compact"][1])
        st1 = st1.copy(); ef1 = s.estimates(); h1 = s.hist()
        st2, _ = s.finish()
        compactions.append(s.kernel_ms()["k_hist_compact"][1])
        st2 = st2.copy(); ef2 = s.estimates(); h2 = s.hist()
        st3, _ = s.finish()
        compactions.append(s.kernel_ms()["k_hist_compact"][1])
        st3 = st3.copy(); ef3 = s.estimates()
        st4, _ = s.finish()
        compactions.append(s.kernel_ms()["k_hist_compact"][1])
        st4 = st4.copy(); ef4 = s.estimates(); h4 = s.hist()
        s.reset()
        st0, summ0 = s.finish()
        compactions.append(s.kernel_ms()["k_hist_compact"][1])
        st0 = st0.copy(); ef0 = s.estimates(); h0 = s.hist()
    assert compactions == [0, 1, 1, 0, 0]
    for st, h in ((st1, h1), (st2, h2), (st3, None), (st4, h4)):
        check_stats(st, exp)
        np.testing.assert_array_equal(st1, st)
        if h is not None:
            check_hist(st, h, exp, exp_hist)
            np.testing.assert_array_equal(h1, h)
    want = oracle_contig_floats(b, est_o).view(np.uint32)
    for ef in (ef1, ef2, ef3, ef4):
        np.testing.assert_array_equal(ef.view(np.uint32), want)
    # no records: the oracle over an empty sample of the same references
    e = to_bamdata(batch_of([]), np.asarray(b.ref_lens, np.int64))
    exp0, exp_hist0, prim0 = O.integer_stats(e, O.FlagFilter(*FF), None, excl)
    assert summ0.num_detected_primary_alignments == prim0 == 0 and summ0.n_records == 0 and summ0.hist_total == 0
    assert len(h0) == len(exp_hist0) == 0
    check_stats(st0, exp0)
    for f in STAT_FIELDS:
        np.testing.assert_array_equal(st0[f], exp0[f], err_msg=f)
    np.testing.assert_array_equal(ef0.view(np.uint32), oracle_contig_floats(e, est_o).view(np.uint32))
    assert not ef0.view(np.uint32).any()


def test_target_mask():
    """One masked-out contig between two others: it has no bins, nothing derives anything for it; with and without estimators set."""
    excl = 75
    b, _ = sample("borders", excl)
    mask = np.asarray([1, 0, 1], np.uint8)
    compare(b, ff=FF, excl=excl, mask=mask)
    exp, exp_hist, prim = O.integer_stats(b, O.FlagFilter(*FF), None, excl, mask)
    live = (exp["seen"] == 1) & (mask != 0)
    with Session(0, FilterConfig(*FF), excl, want_hist=True, want_identity=True) as s:
        s.set_targets(b.ref_lens, mask)
        s.set_estimators(estimators(excl)[0])
        s.push(to_batch(b))
        st, _ = s.finish()
        with pytest.raises(CovError):
            s.estimates()
        check_stats(st, exp, live)
        check_hist(st, s.hist(), exp, exp_hist, live)


def test_genomes():
    """cov_set_genomes over 3 genomes x 2 contigs: the genome kernels read the derived fields of the contigs."""
    excl = 75
    rng = np.random.default_rng(8)
    lens = [5000, 2 * TILE + 1, 140, 3 * TILE, 900, 7000]
    reads = []
    for t, L in enumerate(lens):
        if t != 4:          # one contig without a read: an unobserved length of its genome
            reads += sprinkle(rng, t, 0, L, 120, max_len=400)
    b = to_bamdata(batch_of(reads), np.asarray(lens, np.int64))
    g_of = np.asarray([0, 0, 1, 1, 2, 2], np.int32)
    genomes = ["g0", "g1", "g2"]
    est_e, est_o = estimators(excl)
    exp, exp_hist, prim = O.integer_stats(b, O.FlagFilter(*FF), None, excl)
    with Session(0, FilterConfig(*FF), excl, want_hist=True, want_identity=True) as s:
        s.set_targets(b.ref_lens)
        s.set_genomes(g_of, 3)
        s.set_estimators(est_e)
        s.push(to_batch(b))
        st, _ = s.finish()
        dev = s.genome_estimates()
        gs = s.genome_stats()
        check_stats(st, exp)
        check_hist(st, s.hist(), exp, exp_hist)
        s.finish_genomes()
        np.testing.assert_array_equal(s.genome_estimates().view(np.uint32), dev.view(np.uint32))
    taker = O.CachedTaker(len(est_o))
    O.genome_coverage_with_contig_names([b], ["s"], genomes, {n: int(g) for n, g in zip(b.ref_names, g_of)}, taker, True, O.FlagFilter(*FF), est_o)
    rows = np.zeros((3, len(est_o)), np.float32)
    filled = np.zeros(3, np.int64)
    for entry, cov in taker.coverages[0]:
        rows[entry, filled[entry]] = cov
        filled[entry] += 1
    assert (filled == len(est_o)).all()
    np.testing.assert_array_equal(dev.view(np.uint32), rows.view(np.uint32))
    np.testing.assert_array_equal(gs["reads_in_genome"], np.bincount(g_of, weights=exp["n_pass"]).astype(np.uint64))
    np.testing.assert_array_equal(gs["genome_len"], np.bincount(g_of, weights=lens).astype(np.uint64))
    np.testing.assert_array_equal(gs["n_contigs_seen"], [2, 2, 1])


# ------------------------------------------------------------------ case 9
def test_many_contigs():
    """70 000 contigs of 300 bases, one read each: a lane per contig (k_estimate_lanes derives as its prologue; without estimators
    k_hist_stats does, a lane per contig as well)."""
    excl = 75
    n = 70_000
    rng = np.random.default_rng(9)
    ln = rng.integers(1, 200, n)
    pos = (rng.random(n) * (300 - ln + 1)).astype(np.int64)
    batch = RecordBatch.from_arrays(np.arange(n), pos, np.full(n, 99), np.full(n, 30), np.ones(n), np.ones(n), ln, np.arange(n + 1, dtype=np.uint32),
                                    (ln << 4).astype(np.uint32))
    b = to_bamdata(batch, np.full(n, 300, np.int64))
    oracle = O.integer_stats(b, O.FlagFilter(*FF), None, excl)
    estimator_path(b, oracle, excl)
    with Session(0, FilterConfig(*FF), excl, want_hist=True) as s:
        s.set_targets(b.ref_lens)
        s.push(batch)
        st, _ = s.finish()
        check_stats(st, oracle[0])
        check_hist(st, s.hist(), oracle[0], oracle[1])
