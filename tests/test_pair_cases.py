"""tests/pair_cases.py proved on the oracle alone: every case's claim — the records the reference's pair filter returns, in order, or the
error it ends with — is what oracle.reader_stage gives for the case's sample, and where a case says that two ways of evaluating a threshold
disagree, they are evaluated here in numpy and do.  Nothing of the code under test runs."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import pair_cases as P

f32 = np.float32
CASES = P.all_cases()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_the_claim_is_the_oracles(case):
    b = case.oracle_bam()
    assert O.filter_mode(case.fp)[1], "the pair branch"
    if case.error:
        with pytest.raises(O.OracleError) as ei:
            O.reader_stage(b, case.fp)
        assert ei.value.code == case.error
        return
    order, prim = O.reader_stage(b, case.fp)
    assert [int(i) for i in order] == case.order
    assert prim == int(((b.flag & 0x900) == 0).sum())
    assert 0 < len(case.order) < b.n_records, "deviating pairs among passing ones"


def test_sizes():
    for c in CASES:
        n = c.bam.n_records
        assert n <= {"order": 4400, "chunk": 3700, "table": 1100}.get(c.group, 500), (c.id, n)


@pytest.mark.parametrize("single", [False, True], ids=["pair", "single"])
@pytest.mark.parametrize("thr", P.IDENTITY_THRESHOLDS)
def test_identity_ties(thr, single):
    ties = P.identity_ties(thr)
    assert len(ties["gt"]) >= 3
    if thr in (0.97, 0.99):
        assert len(ties["f64"]) >= 3
    known = {0.90: ("gt", [(50, 5), (60, 6), (100, 10)]), 0.97: ("f64", [(100, 3), (200, 6), (300, 9)]), 0.99: ("f64", [(100, 1), (200, 2), (300, 3)])}
    if thr in known:
        assert set(known[thr][1]) <= set(ties[known[thr][0]])
    c = P.identity_tie(thr, single)
    for variant, rows in c.meta["sets"].items():
        tied = [r for r in rows if r["tie"]]
        assert len(tied) == min(3, len(ties[variant]))
        if not rows:
            continue
        v = P.identity_variants([r["al"] for r in tied], [r["ed"] for r in tied], f32(thr))
        assert (v["ref"] != v[variant]).all()
        assert {r["keep"] for r in rows} == {True, False}, "passing and failing neighbours"
        # the records hold what the claim says: the pair's sums (deletions left out), or the single read's own figures (deletions counted)
        b = c.bam
        for r in rows:
            i1, i2 = r["records"]
            if single:
                assert any(O._aligned_single(b, i) == r["al"] and int(b.nm[i]) == r["ed"] and O._aligned_pair(b, i) == r["al"] - 2 for i in (i1, i2))
            else:
                assert O._aligned_pair(b, i1) + O._aligned_pair(b, i2) == r["al"] and int(b.nm[i1]) + int(b.nm[i2]) == r["ed"]
                assert O._aligned_pair(b, i1) != O._aligned_pair(b, i2)
            assert (i2 in c.order) == r["keep"]


@pytest.mark.parametrize("single", [False, True], ids=["pair", "single"])
@pytest.mark.parametrize("thr", P.PERCENT_THRESHOLDS)
def test_aligned_percent_ties(thr, single):
    ties = P.percent_ties(thr)
    c = P.percent_tie(thr, single)
    b = c.bam
    for variant, rows in c.meta["sets"].items():
        tied = [r for r in rows if r["tie"]]
        assert len(tied) == min(3, len(ties[variant]))
        if not rows:
            continue
        v = P.percent_variants([r["al"] for r in tied], [r["ls"] for r in tied], f32(thr))
        assert (v["ref"] != v[variant]).all()
        assert {r["keep"] for r in rows} == {True, False}
        for r in rows:
            i1, i2 = r["records"]
            if single:
                assert any(O._aligned_single(b, i) == r["al"] and int(b.l_seq[i]) == r["ls"] for i in (i1, i2))
            else:
                assert O._aligned_pair(b, i1) + O._aligned_pair(b, i2) == r["al"] and int(b.l_seq[i1]) + int(b.l_seq[i2]) == r["ls"]
                assert int(b.l_seq[i1]) != int(b.l_seq[i2]), "the sum is split unevenly"
            assert (i2 in c.order) == r["keep"]


def test_aligned_percent_ties_exist():
    """51 (al, l_seq) in l_seq 50..301 where f64 decides otherwise, 11 of them also under multiply-by-reciprocal; both lists are used."""
    f64 = {(thr, t) for thr in P.PERCENT_THRESHOLDS for t in P.percent_ties(thr)["f64"]}
    recip = {(thr, t) for thr in P.PERCENT_THRESHOLDS for t in P.percent_ties(thr)["recip"]}
    assert len(f64) == 51 and len(f64 & recip) == 11
    assert {(0.80, (40, 50)), (0.80, (44, 55)), (0.80, (48, 60)), (0.80, (80, 100))} <= f64 and (0.80, (80, 100)) in recip
    used = {v for thr in P.PERCENT_THRESHOLDS for v, rows in P.percent_tie(thr, False).meta["sets"].items() if rows}
    assert {"f64", "recip"} <= used


@pytest.mark.parametrize("single", [False, True], ids=["pair", "single"])
def test_aligned_length_claims(single):
    c = P.aligned_length(single)
    for r in c.meta["claims"]:
        assert (r["records"][1] in c.order) == r["keep"], r
    by = {r["cigar"]: r["keep"] for r in c.meta["claims"]}
    assert by["100M"] and not by["99M"] and by["90M10D"] == single and by["100="] and by["100X"]
    assert not (by["50M50N"] or by["50M50S"] or by["50M50H"] or by["50M50P"])


@pytest.mark.parametrize("single", [False, True], ids=["pair", "single"])
@pytest.mark.parametrize("min_mapq", [0, 30, 255])
def test_mapq_claims(min_mapq, single):
    c = P.mapq(min_mapq, single)
    kept = {r["mapq"] for r in c.meta["claims"] if r["keep"]}
    for r in c.meta["claims"]:
        assert (r["records"][1] in c.order) == r["keep"], r
    want = {0: {(29, 30), (30, 29), (30, 30), (0, 0), (60, 60)}, 30: {(30, 30), (60, 60)}, 255: set(P.MAPQ_MATES)}[min_mapq]
    assert kept == want


@pytest.mark.parametrize("kind", P.ZERO_KINDS)
def test_zero_length_claims(kind):
    c = P.zero_lengths(kind)
    for r in c.meta["claims"]:
        assert (r["records"][1] in c.order) == r["keep"], r
    assert {r["keep"] for r in c.meta["claims"]} == {True, False}


PARKING_X = {     # every record of name x in file order: (reference, flag, its mate reference is its own)
    "first_away": [(0, 99, False), (0, 147, True)],
    "second_away": [(0, 99, True), (0, 147, False)],
    "abc_first_not_parking": [(0, 99, False), (0, 147, True), (0, 99, True)],
    "abc_all_parking": [(0, 99, True), (0, 147, True), (0, 99, True)],
    "abcd": [(0, 99, True), (0, 147, True), (0, 99, True), (0, 147, True)],
    "abcd_middle_away": [(0, 99, True), (0, 147, False), (0, 99, False), (0, 147, True)],
    "five": [(0, 99, True), (0, 147, True), (0, 99, True), (0, 147, True), (0, 99, True)],
    "five_second_away": [(0, 99, True), (0, 147, False), (0, 99, False), (0, 147, True), (0, 99, True)],
    "two_references": [(0, 99, True), (1, 147, True), (2, 99, False)],
    "secondary_and_improper": [(0, 99 | 0x100, True), (0, 97, True), (0, 99, True), (0, 147 | 0x800, True), (0, 145, True), (0, 147, True), (0, 99 | 0x100, True)],
    "unmapped_flag_with_proper": [(0, 99 | 0x4, True), (0, 147, True)],
}
PARKING_PAIRS = {  # the pairs of name x that come out, as positions in the list above
    "first_away": [], "second_away": [(0, 1)], "abc_first_not_parking": [(1, 2)], "abc_all_parking": [(0, 1)], "abcd": [(0, 1), (2, 3)],
    "abcd_middle_away": [(0, 1)], "five": [(0, 1), (2, 3)], "five_second_away": [(0, 1), (3, 4)], "two_references": [], "secondary_and_improper": [(2, 5)],
    "unmapped_flag_with_proper": [(0, 1)],
}


@pytest.mark.parametrize("kind", P.PARKING_KINDS)
def test_parking_says_what_it_builds(kind):
    """Record by record: name x of every parking case with each record's reference, flag and mate reference, and the pairs of x that come out."""
    c = P.parking(kind)
    b = c.bam
    xs = [i for i, q in enumerate(b.qname) if q == b"x"]
    assert [(int(b.tid[i]), int(b.flag[i]), bool(b.mtid[i] == b.tid[i])) for i in xs] == PARKING_X[kind]
    got = [(xs.index(c.order[k]), xs.index(c.order[k + 1])) for k in range(0, len(c.order), 2) if b.qname[c.order[k]] == b"x"]
    assert got == PARKING_PAIRS[kind]
    if kind == "abcd":      # other pairs' second records between B and D
        between = [i for i in c.order[1::2] if xs[1] < i < xs[3]]
        assert len(between) >= 2 and all(b.qname[i] != b"x" for i in between)


def _lands_at_its_slot(keys, mine, mask):
    """Linear probing fills the same set of slots in whatever order the keys arrive: if the others alone leave my starting slot empty, nobody
    is ever placed there but me."""
    used = set()
    for k in keys:
        if k == mine:
            continue
        h = P.table_slot(k[0], k[1], mask)
        while h in used:
            h = (h + 1) & mask
        used.add(h)
    return P.table_slot(mine[0], mine[1], mask) not in used


def test_deviating_pairs_are_entries_of_two_records_at_their_lanes():
    """Every deviating pair of the judgement and NM cases has a read name of its own, used by exactly its two records (so k_pair_resolve
    judges it, not the list path), and its table entry is looked at in the lane claimed: 0, 31 or 63 of a wave."""
    seen = 0
    for c in CASES:
        lanes = c.meta.get("lanes") or {}
        if not lanes:
            continue
        b = c.bam
        assert c.group in ("judge", "nm") and set(lanes.values()) <= set(P.LANES)
        elig = [i for i in range(b.n_records) if (int(b.flag[i]) & 0x902) == 2 and b.tid[i] == 0]
        mask = P.table_size(b.n_records) - 1
        assert mask == 1023
        key = lambda q: (P.key_k1(P._hash(q)[0]), P.key_k2t(P._hash(q)[1], 0))
        keys = {key(b.qname[i]) for i in elig}
        for name, lane in lanes.items():
            assert sum(1 for i in elig if b.qname[i] == name) == 2, (c.id, name)
            assert P.table_slot(*key(name), mask) & 63 == lane
            assert _lands_at_its_slot(keys, key(name), mask), (c.id, name)
            seen += 1
        if c.group == "judge":
            assert len(lanes) >= 3 and set(lanes.values()) == set(P.LANES)
            claims = c.meta.get("claims") or [r for rows in c.meta["sets"].values() for r in rows]
            assert len(claims) == len(lanes)
            for r in claims:
                assert b.qname[r["records"][0]] == b.qname[r["records"][1]] and b.qname[r["records"][0]] in lanes
    assert seen > 200


def test_output_order_crosses_the_scan_block():
    c = P.output_order()
    o = np.asarray(c.order)
    first, second = o[0::2], o[1::2]
    assert (np.diff(second) > 0).all() and (first < second).all()
    assert not (np.diff(first) > 0).all(), "nested pairs: the first records do not ascend"
    assert ((first < 4096) & (second >= 4096)).sum() >= 2 and c.bam.n_records > 4096 + 100
    ncig = np.diff(c.bam.cigar_off.astype(np.int64))
    assert set(ncig.tolist()) == {1, 3, 5, 7}
    assert 0 < len(o) < 2 * ((c.bam.flag & 0x80) != 0).sum()


def test_table_cases_land_where_they_say():
    c = P.table_equal_first_word()
    groups = {}
    for i, (a, k) in c.meta["over"].items():
        groups.setdefault(a, set()).add((k, P.slot_of(a, k, 0, 1023)))
    assert len(groups) == 2
    for a, ks in groups.items():
        assert len(ks) == 2 and len({s for _, s in ks}) == 1, "two keys, one first word, one starting slot"
    for n in (512, 513):
        for injected in (True, False):
            c = P.table_wrap(n, injected)
            size = c.meta["size"]
            assert size == {512: 1024, 513: 2048}[n] and c.bam.n_records == n
            seen = 0
            for i, q in enumerate(c.bam.qname):
                if q in c.meta["names"]:
                    a, k = (int(c.keys[0][i]), int(c.keys[1][i])) if injected else P._hash(q)
                    assert P.slot_of(a, k, 0, size - 1) >= size - 3
                    seen += 1
            assert seen == 81 and len(set(c.meta["names"])) == 40
    z = P.table_zero_and_one()
    assert sorted(set(z.keys[0].tolist()) & {0, 1}) == [0, 1]


def test_chunk_cuts_fall_where_they_say():
    """The cuts of k_pair_cuts, restated: the cut for target c * 1024 is the first record whose reference lies behind that of record
    c * 1024 - 1."""
    want = {"exactly_1024_then_others": [0, 1024, 1625], "1023_and_1025": [0, 2048, 2048], "3500_two_empty_chunks": [0, 3500, 3500, 3500, 3600],
            "no_reference_at_the_end": [0, 1024, 1054], "triples_in_first_middle_last": [0, 1030, 2054, 3154, 3654]}
    for kind in P.CHUNK_KINDS:
        c = P.chunks(kind)
        key = np.where(c.bam.tid < 0, 0x7FFFFFFF, c.bam.tid).astype(np.int64)
        n = len(key)
        n_chunks = -(-n // 1024)
        cuts = [0] + [n if k == n_chunks or k * 1024 >= n else int(np.searchsorted(key, key[k * 1024 - 1], side="right")) for k in range(1, n_chunks + 1)]
        assert cuts == want[kind], kind
        assert c.knobs == dict(pair_chunk=1024)
    c = P.chunks("triples_in_first_middle_last")
    tri = sorted({int(c.bam.tid[i]) for i, q in enumerate(c.bam.qname) if q.endswith(b".tri")})
    assert tri == [0, 2, 3]
    c = P.chunks("no_reference_at_the_end")
    assert (c.bam.tid[-30:] == -1).all() and c.order[-1] >= 1024, "a pair among the records without a reference"


def test_list_cap_counts():
    for c, listed, cap in ((P.list_cap(False), 64, 64), (P.list_cap(True), 66, 64), (P.list_cap_floor(False), 16, 1), (P.list_cap_floor(True), 19, 1)):
        names, counts = np.unique(np.asarray(c.bam.qname)[(c.bam.flag & 0x902) == 2], return_counts=True)
        assert int(counts[counts > 2].sum()) == listed == c.meta["listed"] and c.knobs == dict(pair_multi_cap=cap)
        assert c.declined == (listed > max(cap, 16)), "a value below 16 is 16"


def test_concatenation_keeps_every_case_apart():
    cs = [c for c in CASES if c.group in ("judge", "park")]
    bam, offs = P.concatenated(cs)
    assert bam.n_records == sum(c.bam.n_records for c in cs) and (np.diff(bam.tid) >= 0).all()
    for c, at in zip(cs, offs):
        order, _ = O.reader_stage(bam, c.fp)
        mine = [int(i) - at for i in order if at <= i < at + c.bam.n_records]
        assert mine == c.order, c.id
