"""k_estimate, k_estimate_lanes, k_genome_estimate and k_genome_estimate_lanes at their decision points, against the reference's estimator
evaluated by the oracle on the contig's own delta array (oracle.estimate_one — independent of csrc/host_coverage.cpp) and, for genomes of
several observed contigs, oracle.genome_coverage_with_contig_names: the same f32 bit for bit, NaN and inf included.  The inputs are the
engineered contigs of tests/edge_inputs.py (tests/test_edge_inputs.py proves on the CPU that each stands where it claims): a prefix sum
exactly on min_index or max_index, the start and end bins on either side of a 64-bin batch, 96 and 97 bins, unobserved contigs of exactly
2 x excl bases.  Every case runs with a wave per entry and with a lane per entry (COVERM_EST_LANES), beside a contig without reads and a
contig shorter than the end exclusion."""
import functools

import numpy as np
import pytest

from coverm_amd.engine import FilterConfig, Session
from coverm_amd.host import CoverageEstimator as E
from oracle import oracle as O
from tests import edge_inputs as X
from tests.test_gpu_abi_parity import to_batch

pytestmark = pytest.mark.gpu

FF = (True, True, False)
OFF = O.FlagFilter(*FF)


def oracle_param(e):
    return O.EstParam(e.kind, e.min_fraction_covered_bases, e.contig_end_exclusion, e.exclude_mismatches, e.trim_min, e.trim_max)


def trimmed_set(excl, trims):
    trims = list(dict.fromkeys(list(trims) + list(X.TRIM_PAIRS)))
    est = [E.new_estimator_trimmed_mean(a, b, 0.0, excl) for a, b in trims]
    est += [E.new_estimator_trimmed_mean(0.1, 0.9, 0.1, excl), E.new_estimator_trimmed_mean(X.TRIM[0], X.TRIM[1], 0.76, excl)]
    assert len(est) <= 16
    return est


def other_set(excl):
    return [E.new_estimator_mean(0.0, excl, False), E.new_estimator_mean(0.1, excl, True), E.new_estimator_variance(0.0, excl),
            E.new_estimator_variance(0.3, excl), E.new_estimator_covered_fraction(0.0), E.new_estimator_covered_fraction(0.76),
            E.new_estimator_covered_bases(0.1), E.new_estimator_rpkm(0.0), E.new_estimator_rpkm(0.5), E.new_estimator_length(),
            E.new_estimator_read_count(), E.new_estimator_reads_per_base(), E.new_estimator_anir()]


def contig_reference(b, excl, est):
    """The oracle's floats, contigs x estimators: estimate_one on the contig's delta array; a contig without a considered record prints
    zeros (contig.rs: print_zero_coverage)."""
    st = O.integer_stats(b, OFF, None, excl)[0]
    out = np.zeros((len(b.ref_names), len(est)), np.float32)
    params = [oracle_param(e) for e in est]
    for t in np.nonzero(st["n_pass"] > 0)[0]:
        ud = O.contig_deltas(b, OFF, int(t))
        for k, p in enumerate(params):
            out[t, k] = O.estimate_one(p, ud, int(st["n_primary"][t]), int(st["sum_nm"][t]) - int(st["sum_indel"][t]), float(st["id_primary"][t]))
    return out


def contig_device(b, excl, est):
    with Session(0, FilterConfig(*FF), excl, want_hist=True, want_identity="primary") as s:
        s.set_targets(b.ref_lens)
        s.set_estimators(est)
        s.push(to_batch(b))
        s.finish()
        return s.estimates()


def assert_bits(dev, exp, rows, est, what):
    bad = np.argwhere(dev.view(np.uint32) != exp.view(np.uint32))
    assert bad.size == 0, "%s: %d floats differ; first: %s, estimator %d (kind %d, trim %r %r, min fraction %r): device %r (%#x) oracle %r (%#x)" % (
        what, len(bad), rows(bad[0][0]), bad[0][1], est[bad[0][1]].kind, est[bad[0][1]].trim_min, est[bad[0][1]].trim_max,
        est[bad[0][1]].min_fraction_covered_bases, dev[tuple(bad[0])], dev.view(np.uint32)[tuple(bad[0])], exp[tuple(bad[0])], exp.view(np.uint32)[tuple(bad[0])])


@functools.lru_cache(maxsize=None)
def family(name, excl):
    b, where = X.family_sample(name, excl)
    sets = [trimmed_set(excl, [c.trim for c in where.values()]), other_set(excl)]
    return b, where, [(est, contig_reference(b, excl, est)) for est in sets]


@pytest.mark.parametrize("lanes", [0, 1])
@pytest.mark.parametrize("excl", [0, 75])
@pytest.mark.parametrize("name", sorted(X.FAMILIES))
def test_contig_entries(name, excl, lanes, monkeypatch):
    """start: the start bin at lanes 0, 1, 62 .. 65, 95 .. 97, 127, 128 and 200 with its prefix on min_index and one above; end: the end bin
    on the start bin, next to it, at lane 0 of the next batch, three batches on, missing; bins: 2 .. 129 occupied bins, 300 and 600 sparse;
    pairs: equal indices, min > max, trim_min 0 over an empty bin 0; bin0_extra: untouched tiles, the border through a segment;
    variance: a window covered everywhere, one uncovered base, T < 3."""
    monkeypatch.setenv("COVERM_EST_LANES", str(lanes))
    b, where, sets = family(name, excl)
    for est, exp in sets:
        dev = contig_device(b, excl, est)
        assert_bits(dev, exp, lambda t: where[t].name if t in where else b.ref_names[t], est, "%s excl %d lanes %d" % (name, excl, lanes))


@functools.lru_cache(maxsize=None)
def fraction_sample(excl):
    c = X.min_fraction_case()
    b = X.concat([X.bare(700), c.bam(excl), X.short_with_reads()])
    st = O.integer_stats(b, OFF, None, excl)[0]
    one = np.float32(1)
    win = np.float32(int(st["win_covered"][1])) / np.float32(c.T)                     # covered / T as the reference computes it, in f32
    full = np.float32(int(st["full_covered"][1])) / np.float32(int(b.ref_lens[1]))
    sets = []
    for f, make in ((win, [lambda m: E.new_estimator_mean(m, excl, True), lambda m: E.new_estimator_trimmed_mean(0.05, 0.95, m, excl),
                           lambda m: E.new_estimator_variance(m, excl)]),
                    (full, [E.new_estimator_covered_fraction, E.new_estimator_covered_bases, E.new_estimator_rpkm])):
        steps = [float(np.nextafter(f, -one)), float(f), float(np.nextafter(f, one + one))]      # one f32 step below, at, one above
        sets.append([mk(m) for mk in make for m in steps])
    return b, [(est, contig_reference(b, excl, est)) for est in sets]


@pytest.mark.parametrize("lanes", [0, 1])
@pytest.mark.parametrize("excl", [0, 75])
def test_min_covered_fraction_at_the_fraction_itself(excl, lanes, monkeypatch):
    """The fraction exactly at covered / T as computed in f32 and one f32 step on either side, for the mean without mismatches, the trimmed
    mean, the variance (window fraction) and covered fraction, covered bases, rpkm (whole-contig fraction)."""
    monkeypatch.setenv("COVERM_EST_LANES", str(lanes))
    b, sets = fraction_sample(excl)
    for est, exp in sets:
        assert (exp[1][0::3] != 0).all() and (exp[1][1::3] != 0).all() and (exp[1][2::3] == 0).all()      # zero from one step above the fraction on
        assert_bits(contig_device(b, excl, est), exp, lambda t: b.ref_names[t], est, "min fraction excl %d lanes %d" % (excl, lanes))


LONG_EST = lambda excl: [E.new_estimator_trimmed_mean(0.05, 0.95, 0.0, excl), E.new_estimator_trimmed_mean(0.0, 1.0, 0.0, excl),       # noqa: E731
                         E.new_estimator_mean(0.0, excl, True), E.new_estimator_variance(0.0, excl), E.new_estimator_covered_fraction(0.0),
                         E.new_estimator_length(), E.new_estimator_reads_per_base(), E.new_estimator_rpkm(0.0)]


@functools.lru_cache(maxsize=None)
def long_sample(excl):
    b = X.concat([X.bare(10), X.long_contig_case().bam(excl), X.short_with_reads()])
    est = LONG_EST(excl)
    return b, est, contig_reference(b, excl, est)


@pytest.mark.parametrize("lanes", [0, 1])
@pytest.mark.parametrize("excl", [0, 75])
def test_window_longer_than_f32_holds(excl, lanes, monkeypatch):
    """A window of 2^24 + 3 bases: float(T) rounds, in the indices and in every division by T."""
    monkeypatch.setenv("COVERM_EST_LANES", str(lanes))
    b, est, exp = long_sample(excl)
    assert_bits(contig_device(b, excl, est), exp, lambda t: b.ref_names[t], est, "long contig excl %d lanes %d" % (excl, lanes))


# ------------------------------------------------------------------------------------------------ genome entries
def genome_sets(excl):
    return [[E.new_estimator_trimmed_mean(a, b, 0.0, excl) for a, b in dict.fromkeys([X.GENOME_TRIM] + list(X.TRIM_PAIRS))] +
            [E.new_estimator_trimmed_mean(X.GENOME_TRIM[0], X.GENOME_TRIM[1], 0.2, excl)],
            [E.new_estimator_mean(0.0, excl, False), E.new_estimator_mean(0.1, excl, True), E.new_estimator_variance(0.0, excl),
             E.new_estimator_covered_fraction(0.0), E.new_estimator_covered_bases(0.3), E.new_estimator_rpkm(0.0), E.new_estimator_length(),
             E.new_estimator_read_count(), E.new_estimator_reads_per_base(), E.new_estimator_anir()]]


@functools.lru_cache(maxsize=None)
def genomes(excl):
    b, g_of, n_genomes, single = X.genome_sample(excl)
    st = O.integer_stats(b, OFF, None, excl)[0]
    names = ["g%d" % g for g in range(n_genomes)]
    c2g = {n: int(g) for n, g in zip(b.ref_names, g_of) if g >= 0}
    refs = []
    for est in genome_sets(excl):
        params = [oracle_param(e) for e in est]
        taker = O.CachedTaker(len(est))
        O.genome_coverage_with_contig_names([b], ["s"], names, c2g, taker, True, OFF, params)
        printed = np.zeros((n_genomes, len(est)), np.float32)          # what the scan prints: a coverage that is not above zero prints as zero
        for j, (entry, cov) in enumerate(taker.coverages[0]):
            printed[entry, j % len(est)] = cov
        exact = {}                                                      # genomes of one observed contig: the estimator's own float
        for g, (_, tid, un) in single.items():
            ud = O.contig_deltas(b, OFF, tid)
            exact[g] = np.asarray([O.estimate_one(p, ud, int(st["n_pass"][tid]), int(st["sum_nm"][tid]) - int(st["sum_indel"][tid]),
                                                  float(st["id_nonsupp"][tid]), unobserved=un) for p in params], np.float32)
        refs.append((est, printed, exact))
    return b, g_of, n_genomes, single, refs


@pytest.mark.parametrize("lanes", [0, 1])
@pytest.mark.parametrize("excl", [0, 75])
def test_genome_entries(excl, lanes, monkeypatch):
    """One staircase contig with unobserved contigs of 1, 2 x excl - 1, 2 x excl, 2 x excl + 1 and 5 000 bases around it, the merged bin 0
    on either side of min_index and max_index; two observed contigs with different bin counts and an observed contig without a window; a
    genome of 300 contigs (two segments); with a wave per genome and with a lane per genome."""
    monkeypatch.setenv("COVERM_EST_LANES", str(lanes))
    b, g_of, n_genomes, single, refs = genomes(excl)
    batch = to_batch(b)
    for est, printed, exact in refs:
        with Session(0, FilterConfig(*FF), excl, want_hist=True, want_identity="nonsupp") as s:
            s.set_targets(b.ref_lens)
            s.set_genomes(g_of, n_genomes)
            s.set_estimators(est)
            s.push(batch)
            s.finish_genomes()
            assert s.genome_kernel_ms()[1] > 0, "the genome kernels did not run"
            dev = s.genome_estimates()
        what = "genomes excl %d lanes %d" % (excl, lanes)
        for g, row in exact.items():
            assert_bits(dev[g:g + 1], row[None, :], lambda _: single[g][0].name, est, what)
        shown = np.where(dev > 0, dev, np.float32(0))
        assert_bits(shown, printed, lambda g: "genome %d" % g, est, what)
