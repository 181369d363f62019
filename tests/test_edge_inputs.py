"""tests/edge_inputs.py on the CPU, against the reference alone (the oracle's integer statistics, numpy's f32, Python's floats): every
engineered case has the property it is named for — what keeps test_gpu_estimator_edges.py and test_gpu_identity_edges.py from passing for
the wrong reason.  No device code runs or is imported here."""
from fractions import Fraction

import numpy as np
import pytest

from oracle import oracle as O
from tests import edge_inputs as X

FF = O.FlagFilter(True, True, False)


def window_hist(b, excl, tid):
    st, hist, _ = O.integer_stats(b, FF, None, excl)
    off = int(st["hist_off"][tid])
    return hist[off:off + int(st["hist_len"][tid])], st


def test_staircase_has_the_histogram_asked_for():
    counts = [7] + [3] * 130
    b = X.staircase(counts)
    h, st = window_hist(b, 0, 0)
    assert b.n_records == 8515 and int(st["hist_len"][0]) == 131
    np.testing.assert_array_equal(h, np.asarray(counts, np.uint64))
    sparse = {0: 11, 2: 5, 599: 4}
    for excl in (0, 75):
        b = X.staircase(sparse, excl, pad_left=3, mid=2, mid_after=2)
        assert b.n_records == 601 and int(b.ref_lens[0]) == 20 + 2 * excl
        np.testing.assert_array_equal(window_hist(b, excl, 0)[0], X.dense(sparse))
    # the border cuts through the first segment: the window's histogram is the same, the bases outside it are covered
    b = X.staircase({0: 4, 1: 10, 3: 2}, 75, cut_left=30)
    h, st = window_hist(b, 75, 0)
    np.testing.assert_array_equal(h, [4, 10, 0, 2])
    assert int(st["full_covered"][0]) == 12 + 30 and int(st["win_covered"][0]) == 12


@pytest.mark.parametrize("excl", [0, 75])
@pytest.mark.parametrize("family", sorted(X.FAMILIES))
def test_estimator_cases_stand_where_they_claim(family, excl):
    b, where = X.family_sample(family, excl)
    st, hist, _ = O.integer_stats(b, FF, None, excl)
    assert int(st["n_pass"][0]) == 0                                          # the contig without reads in front
    for tid, c in where.items():
        assert int(b.ref_lens[tid]) == c.T + 2 * excl
        h = hist[int(st["hist_off"][tid]):int(st["hist_off"][tid]) + int(st["hist_len"][tid])]
        np.testing.assert_array_equal(h, X.dense(c.counts), err_msg=c.name)
        # the indices in f32, as the reference computes them, and the walk over the ORACLE's histogram
        T = np.float32(c.T)
        mn, mx = int(np.floor(np.float32(c.trim[0]) * T)), int(np.ceil(np.float32(c.trim[1]) * T))
        P = np.cumsum(h.astype(np.int64))
        assert P[-1] == c.T
        if c.s is None:
            continue
        s = int(np.argmax(P >= mn))
        assert s == c.s and (s == 0 or P[s - 1] == mn - 1), c.name
        if c.ps is not None:
            assert P[s] - mn == c.ps, c.name
        if c.e is None:
            assert P[-1] <= mx, c.name                                         # no end bin at all
        elif c.e == c.s:
            assert P[s] > mx, c.name                                           # the first bin to reach min_index already exceeds max_index
        else:
            assert P[c.e] > mx and P[c.e - 1] <= mx and P[c.e - 1] - mx == c.pe, c.name
        if c.plast is not None:
            assert P[-1] - mx == c.plast, c.name


def test_the_families_hold_the_cases_of_the_issue():
    names = {c.name for f in X.FAMILIES.values() for c in f()}
    for s in (0, 1, 62, 63, 64, 65, 95, 96, 97, 127, 128, 200):
        assert {"start_s%d_dv0" % s, "start_s%d_dv1" % s} <= names
    assert {"end_s63_same", "end_s63_next_ev0", "end_s63_next_ev1", "end_s1_lane0_ev0", "end_s70_3batches_ev1", "end_s1_none_last_is_max",
            "end_s70_trim_max_one"} <= names
    bins = {int(X.dense(c.counts).size) for c in X.bin_count_cases()}
    assert bins == {2, 64, 65, 96, 97, 128, 129, 300, 600}
    by_name = {c.name: c for f in X.FAMILIES.values() for c in f()}
    assert by_name["end_s63_next_ev0"].e == 64                                  # the start bin at lane 63, the end bin at lane 0 of the next batch
    c = by_name["end_s70_3batches_ev0"]
    assert c.e // 64 == c.s // 64 + 3 and all(d not in c.counts for d in range(c.s + 3, 128))        # a run of empty bins between s and e
    for T in (X.T0, X.T0 + 1):
        mn, mx = X.f32_indices(T, 0.5, 0.5)
        assert mx - mn == T - X.T0                                              # equal indices: the mean divides by zero
    assert by_name["pair_min0_empty_bin0"].counts[0] == 0
    mn, mx = X.f32_indices(X.T0, 0.9, 0.1)
    assert mn > mx
    assert X.f32_indices(X.T0, *X.NO_END)[1] == X.T0
    # bin 0 of the untouched-tiles case: at least three whole 1024-base tiles in the middle and at the end, whatever their alignment
    c = by_name["tiles_untouched"]
    assert c.stair["mid"] >= 4 * 1024 and c.counts[0] - c.stair["mid"] - c.stair["pad_left"] >= 4 * 1024
    c = X.long_contig_case()
    assert c.T == (1 << 24) + 3 and float(np.float32(c.T)) == (1 << 24) + 4     # f32(T) rounds


def test_variance_and_fraction_cases():
    v = {c.name: c for c in X.variance_cases()}
    assert min(d for d, n in v["covered_everywhere"].counts.items() if n) == 3
    assert v["one_uncovered_base"].counts[0] == 1 and v["one_uncovered_base"].T == v["covered_everywhere"].T
    assert (v["T1"].T, v["T2"].T, v["T3"].T) == (1, 2, 3)
    c = X.min_fraction_case()
    for excl in (0, 75):
        st = O.integer_stats(c.bam(excl), FF, None, excl)[0]
        assert int(st["win_covered"][0]) == 2766 and int(st["full_covered"][0]) == 2766 and int(st["sum_nm"][0]) == c.bam(excl).n_records


def test_tie_at_and_the_search():
    assert X.tie_at(0.5 + 2.0 ** -52, 1) and not X.tie_at(0.5, 1) and not X.tie_at(0.5 + 2.0 ** -51, 1) and X.tie_at(0.5 + 2.0 ** -51, 2)
    assert not X.tie_at(1.0, 5) and not X.tie_at(0.0, 5)
    assert len(X.tie_pairs(1)) == 187363 and len(X.tie_pairs(9)) == 238
    for e in range(1, 10):
        p = X.tie_pairs(e)
        assert len(p) and all(X.tie_at(X.identity(int(a), int(m)), e) for a, m in p[:50])
    assert X.wide_tie_pair(10) == (4097, 32) and X.wide_tie_pair(12) == (16385, 2) and X.wide_tie_pair(17) == (524289, 4)


def test_tie_cases_meet_the_sum_in_their_binade_and_tell_the_roundings_apart():
    parities, rounded_up, n_cases = set(), set(), 0
    for e in X.TIE_BINADES:
        b, cases = X.tie_sample(e)
        places = [p for p, _, _, _ in cases]
        assert places == [p for p in X.TIE_PLACES if e < 10 or not p.startswith("head")]
        for place, values, first, ti in cases:
            n_cases += 1
            assert (b.tid == b.tid[first]).sum() == len(values) and int(np.argmax(b.tid == b.tid[first])) == first
            sums, ties = X.replay(values)
            assert ties == [ti], (e, place, ties, ti)                           # the one tie of the chain is the record built for it
            before = sums[ti - 1]
            assert X.binade(before) == e and X.binade(sums[ti]) == e and X.tie_at(X.identity(*values[ti]), e)
            parities.add(X._bits(before) & 1)
            rounded_up.add(Fraction(sums[ti]) > Fraction(before) + Fraction(X.identity(*values[ti])))
            assert X.binade(sums[-1]) == e, (e, place)                          # the contig ends in the same binade
            flipped = X.replay(values, flip_ties=True)[0]
            assert X._bits(flipped[-1]) != X._bits(sums[-1]), (e, place)        # the other rounding ends in other bits
            # where the tie stands in the sample
            g, start, end = first + ti, first, first + len(values)
            k0, k1 = -(-start // X.ID_CH), end // X.ID_CH                       # interior chunks [k0, k1)
            assert k0 < k1
            if place == "chunk_first":
                assert g % X.ID_CH == 0 and k0 <= g // X.ID_CH < k1
            elif place == "chunk_last":
                assert g % X.ID_CH == X.ID_CH - 1 and k0 <= g // X.ID_CH < k1
            elif place in ("lane0", "lane63"):
                assert g % 64 == (0 if place == "lane0" else 63) and g % X.ID_CH not in (0, X.ID_CH - 1) and k0 <= g // X.ID_CH < k1
            elif place.startswith("head"):
                assert g < k0 * X.ID_CH and (g - start) % 64 == (0 if place == "head_lane0" else 63)
            else:
                assert g >= k1 * X.ID_CH
            if place != "tail":
                assert len(values) - ti - 1 >= X.ID_CH
                if e >= 10:                                                     # where 1024 addends fit into the binade they are fillers
                    assert all(nm not in (0, X.FILLER_ALIGNED) for _, nm in values[ti + 1:ti + 1 + X.ID_CH])
    assert parities == {0, 1} and rounded_up == {False, True} and n_cases == 4 * 7 + 2 * 5


def test_power_of_two_at_the_end_of_a_chunk():
    values = X.power_of_two_values()
    sums = X.replay(values)[0]
    assert sums[2 * X.ID_CH - 1] == 2.0 ** 11 and sums[4 * X.ID_CH - 1] == 2.0 ** 12       # after chunk 1, after chunk 3 (the contig starts at record 0)
    for start, lane in ((0, 63), (1, 0)):
        b = X.power_of_two_sample(start)
        first = int(np.argmax(b.tid == b.tid[-1]))
        assert first == start
        for k in (10, 11, 12):
            g = first + (1 << k) - 1                                            # the record that lifts the sum to 2^k
            assert sums[g - first] == 2.0 ** k and g % 64 == lane


def test_layout_sample():
    b, spans = X.layout_sample()
    assert sorted(n for _, n in spans) == [1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 3073]
    assert np.array_equal(np.bincount(b.tid), [n for _, n in spans])
    firsts = {a % X.ID_CH for a, _ in spans}
    assert {0, 1, 1023} <= firsts
    assert [a % X.ID_CH for a, n in spans if n == 2048] == [0]                  # no head and no tail
    assert any(a // X.ID_CH == (a + n - 1) // X.ID_CH for a, n in spans if n > 1)          # inside a chunk
    assert any(a // X.ID_CH != (a + n - 1) // X.ID_CH and -(-a // X.ID_CH) >= (a + n) // X.ID_CH for a, n in spans)      # straddles a border, no whole chunk


def test_batches_and_uncounted_samples():
    for n_chunks in (64, 65, 129):
        b, values = X.batches_sample(n_chunks)
        first = int(np.argmax(b.tid == 1))
        assert first == 3 and (first + len(values)) // X.ID_CH - 1 == n_chunks
    total = sum(X.identity(*v) for v in X.batches_sample(129)[1])
    assert X.binade(total) == 17
    b, values, flags = X.uncounted_sample()
    assert {0x800, 0x100, 0x4} == set(flags.values())
    at = {(3 + i) % X.ID_CH for i in flags}
    assert {0, X.ID_CH - 1} <= at                                                 # on both sides of a chunk border
    neg = next(i for i, v in enumerate(values) if v[1] > v[0])
    counted = [v for i, v in enumerate(values[:neg]) if i not in flags]
    assert X.replay(counted)[0][-1] > 4096 and 1 <= (3 + neg) // X.ID_CH < (3 + len(values)) // X.ID_CH
    assert any(v == X.ZERO for v in values)


@pytest.mark.parametrize("excl", [0, 75])
def test_genome_cases_put_the_unobserved_bases_where_they_claim(excl):
    b, g_of, n_genomes, single = X.genome_sample(excl)
    st, hist, _ = O.integer_stats(b, FF, None, excl)
    assert len(g_of) == len(b.ref_names) and n_genomes == len(single) + 4
    assert sorted(X.unobserved_lengths(75)) == [1, 149, 150, 151, 5000]
    for g, (merged, tid, un) in single.items():
        mine = np.nonzero(g_of == g)[0]
        assert list(mine[st["n_pass"][mine] > 0]) == [tid] and mine[0] < tid < mine[-1]      # unobserved contigs in front of it and behind it
        assert sorted(int(b.ref_lens[t]) for t in mine if t != tid) == sorted(un)
        U = sum(n if n < 2 * excl else n - 2 * excl for n in un)
        h = hist[int(st["hist_off"][tid]):int(st["hist_off"][tid]) + int(st["hist_len"][tid])].astype(np.int64)
        h[0] += U                                                                # counts[0] += unobserved (estimators.rs:596)
        np.testing.assert_array_equal(h, X.dense(merged.counts).astype(np.int64))
        T = np.float32(h.sum())
        mn, mx = int(np.floor(np.float32(merged.trim[0]) * T)), int(np.ceil(np.float32(merged.trim[1]) * T))
        P = np.cumsum(h)
        s = int(np.argmax(P >= mn))
        assert s == merged.s and (s == 0 or P[0] == mn - 1), merged.name
        if merged.ps is not None:
            assert P[s] - mn == merged.ps
        if merged.e == merged.s:
            assert P[0] > mx
        else:
            assert P[merged.e] > mx and P[merged.e - 1] - mx == merged.pe
    big = np.nonzero(g_of == len(single) + 1)[0]
    seen = np.nonzero(st["n_pass"][big] > 0)[0]
    assert len(big) == 300 and seen.min() < 256 <= seen.max() and {255, 256} <= set(seen) and (st["n_pass"][big][6:100] == 0).all()
    assert len({int(st["hist_len"][t]) for t in big[seen]}) > 3                  # different bin counts: the merged count is the largest
    two = np.nonzero(g_of == len(single))[0]
    assert {70, 130} <= {int(x) for x in st["hist_len"][two]}                    # two observed contigs with different bin counts
    short = [t for t in two if st["n_pass"][t] > 0 and b.ref_names[t].endswith("short")]
    assert len(short) == 1 and (excl == 0 or int(st["hist_len"][short[0]]) == 0)     # reads and, with the exclusion, no window
