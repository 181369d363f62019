"""Inputs that take the device pair filter (cov_pair_filter_apply: csrc/pair_kernels.hip.h and its driver) through its decision points one
by one: every builder returns one small sample, the filter parameters, and what it claims the reference's filter (filter.rs:117-336) returns
for it — the record indices in output order, or the error.  tests/test_pair_cases.py proves every claim with the oracle alone;
tests/test_gpu_pair_filter_edges.py compares the device with the oracle on the same samples.

Also here: the join key, its slot and the table size (csrc/pair_key_core.h) stated a second time in plain Python integers.  The table cases
place keys in chosen slots with this statement; tests/test_pair_key_core.py holds the two statements against each other."""
import functools
import re
import struct
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from oracle import bamio
from oracle import oracle as O
from tests import namehash

f32 = np.float32
M64 = (1 << 64) - 1


# ---------------------------------------------------------------------------------------------- the key, the slot, the table size
def key_k1(qh1):
    return qh1 if qh1 else 1


def key_k2t(qh2, tid):
    return (qh2 & 0xFFFFFFFF) | (((tid + 2) & 0xFFFFFFFF) << 32)


def table_slot(k1, k2t, mask):
    x = k1 ^ ((k2t * 0x9E3779B97F4A7C15) & M64)
    x ^= x >> 29
    return x & 0xFFFFFFFF & mask


def table_size(n_records):
    cc = 1024
    while cc < 2 * n_records:
        cc *= 2
    return cc


def slot_of(qh1, qh2, tid, mask):
    return table_slot(key_k1(qh1), key_k2t(qh2, tid), mask)


def key_name(qh1, qh2):
    """The read name the oracle is given for an injected key: the key's bytes after the 0 -> 1 rule, so that "same name" to the oracle is
    "same key" to the device."""
    return struct.pack("<QI", key_k1(int(qh1)), int(qh2))


@functools.lru_cache(maxsize=None)
def _hash(name):
    return namehash.name_hash(name)


def name_with(prefix, want, tid=0, mask=1023, taken=()):
    """The first name prefix.j whose key starts its probe run at a slot `want` accepts."""
    for j in range(1 << 20):
        n = b"%s.%d" % (prefix, j)
        if n in taken:
            continue
        k1, k2 = _hash(n)
        if want(slot_of(k1, k2, tid, mask)):
            return n
    raise AssertionError("no name found")


LANES = (0, 31, 63)


def lane_name(prefix, k, tid=0, avoid=()):
    """A name of its own for every k whose entry k_pair_resolve looks at in lane 0, 31 or 63 of a wave (the slot's low six bits, whatever the
    table's size).  avoid: starting slots (of a table of 1 024 entries, which has 16 slots per lane) of the sample's other names, none of
    which may be this name's; tests/test_pair_cases.py shows that no other key's probe run reaches the slot either."""
    lane = LANES[k % 3]
    return name_with(b"%s%d" % (prefix, k), lambda s: (s & 63) == lane and s not in avoid, tid)


@functools.lru_cache(maxsize=None)
def fill_slots(n=120):
    """Where the ordinary pairs f0 .. f(n-1) start in a table of 1 024 entries."""
    return frozenset(slot_of(*_hash(b"f%d" % k), 0, 1023) for k in range(n))


# ---------------------------------------------------------------------------------------------- samples
OPS = {c: i for i, c in enumerate("MIDNSHP=X")}


def cigar_words(text):
    return [(int(n) << 4) | OPS[c] for n, c in re.findall(r"(\d+)([MIDNSHP=X])", text)]


def params(proper=False, **kw):
    """FilterParameters with the percentages as the f32 the command line passes."""
    for k in list(kw):
        if "percent" in k:
            kw[k] = float(f32(kw[k]))
    return O.FilterParameters(O.FlagFilter(not proper, True, False), **kw)


@dataclass
class Case:
    id: str
    group: str                              # judge, park, nm, order, table, chunk, cap
    bam: bamio.BamData
    fp: O.FilterParameters
    order: Optional[list] = None            # claimed output: record indices, first record then second, by second record
    error: Optional[int] = None             # or the claimed error: 2 = NM absent, 3 = NM of a signed type
    knobs: dict = field(default_factory=dict)
    keys: Optional[tuple] = None            # (qh1, qh2) to inject with cov_set_mates
    declined: bool = False                  # the device hands the file to the CPU reader
    meta: dict = field(default_factory=dict)

    def oracle_bam(self):
        """What the oracle reads: the sample, with every read name replaced by its injected key where keys are injected."""
        if self.keys is None:
            return self.bam
        b = self.bam
        names = [key_name(a, c) for a, c in zip(*self.keys)]
        return bamio.BamData(b.ref_names, b.ref_lens, b.tid, b.pos, b.flag, b.mapq, b.l_seq, b.nm, b.nm_kind, b.cigar_off, b.cigar, b.mtid, b.mpos, b.tlen,
                             names, b.header_text)


class Sample:
    """Records in file order; keep(i1, i2) claims a returned pair."""

    def __init__(self, n_refs=1, ref_len=10_000_000):
        self.n_refs, self.ref_len, self.rows, self.kept, self.n_fill, self.lanes = n_refs, ref_len, [], [], 0, {}

    def lname(self, prefix, k):
        """The name of the k-th deviating pair of a sample on one reference: see lane_name."""
        taken = {slot_of(*_hash(n), 0, 1023) for n in self.lanes}
        n = lane_name(prefix, k, 0, fill_slots() | taken)
        self.lanes[n] = LANES[k % 3]
        return n

    def rec(self, name, tid=0, flag=99, mapq=30, nm=0, cigar="100M", l_seq=None, mtid=None, nm_kind=bamio.NM_UNSIGNED):
        w = cigar_words(cigar) if isinstance(cigar, str) else list(cigar)
        if l_seq is None:
            l_seq = sum(x >> 4 for x in w if (x & 15) in (0, 1, 4, 7, 8))
        assert not self.rows or (0x7FFFFFFF if tid < 0 else tid) >= (0x7FFFFFFF if self.rows[-1][1] < 0 else self.rows[-1][1]), "records sorted by reference"
        self.rows.append((name if isinstance(name, bytes) else name.encode(), tid, flag, mapq, nm, w, l_seq, tid if mtid is None else mtid, nm_kind))
        return len(self.rows) - 1

    def keep(self, i1, i2):
        self.kept.append((i1, i2))

    def pair(self, name, keep, a=None, b=None, tid=0):
        """Two adjacent records of one name (flags 99 and 147); a, b: what differs from an ordinary record."""
        i1 = self.rec(name, tid, **dict(dict(flag=99), **(a or {})))
        i2 = self.rec(name, tid, **dict(dict(flag=147), **(b or {})))
        if keep:
            self.keep(i1, i2)
        return i1, i2

    def fill(self, n, tid=0, every=7):
        """n ordinary passing pairs (every `every`-th with a CIGAR of three words)."""
        for _ in range(n):
            k = self.n_fill
            self.n_fill += 1
            c = "60M2I38M" if k % every == 0 else "100M"
            self.pair(b"f%d" % k, True, dict(cigar=c), dict(cigar=c), tid)

    def order(self):
        return [i for p in sorted(self.kept, key=lambda p: p[1]) for i in p]

    def bam(self):
        r = self.rows
        n = len(r)
        coff = np.zeros(n + 1, np.uint32)
        np.cumsum([len(x[5]) for x in r], out=coff[1:])
        z = np.zeros(n, np.int32)
        return bamio.BamData(["r%d" % t for t in range(self.n_refs)], np.full(self.n_refs, self.ref_len, np.int64), np.asarray([x[1] for x in r], np.int32),
                             (100 + 10 * np.arange(n)).astype(np.int32), np.asarray([x[2] for x in r], np.uint16), np.asarray([x[3] for x in r], np.uint8),
                             np.asarray([x[6] for x in r], np.int32), np.asarray([x[4] for x in r], np.uint32), np.asarray([x[8] for x in r], np.uint8), coff,
                             np.asarray([w for x in r for w in x[5]], np.uint32), np.asarray([x[7] for x in r], np.int32), z.copy(), z.copy(), [x[0] for x in r], "")

    def case(self, id, group, fp, error=None, **kw):
        kw["meta"] = dict(kw.get("meta") or {}, lanes=dict(self.lanes))
        return Case(id, group, self.bam(), fp, None if error else self.order(), error, **kw)


def spread(items, n=3):
    """First, middle and last of a list (all of it when it is no longer than n)."""
    items = list(items)
    if len(items) <= n:
        return items
    return [items[0], items[len(items) // 2], items[-1]]


# ---------------------------------------------------------------------------------------------- judgement: thresholds
IDENTITY_THRESHOLDS = (0.90, 0.95, 0.97, 0.99)
PERCENT_THRESHOLDS = (0.80, 0.90, 0.95)


def identity_variants(al, ed, thr):
    """The reference's expression and the two it must not be mistaken for, over arrays of aligned length and edit distance; thr: an f32."""
    al, ed = np.asarray(al), np.asarray(ed)
    v = f32(1.0) - ed.astype(f32) / al.astype(f32)
    return dict(ref=v >= f32(thr), gt=v > f32(thr), f64=1.0 - ed.astype(np.float64) / al.astype(np.float64) >= float(f32(thr)))


def percent_variants(al, ls, thr):
    al, ls = np.asarray(al), np.asarray(ls)
    v = al.astype(f32) / ls.astype(f32)
    return dict(ref=v >= f32(thr), gt=v > f32(thr), f64=al.astype(np.float64) / ls.astype(np.float64) >= float(f32(thr)),
                recip=al.astype(f32) * (f32(1.0) / ls.astype(f32)) >= f32(thr))


@functools.lru_cache(maxsize=None)
def identity_ties(thr):
    """{variant: [(al, ed)]} over aligned 50..300, edit distance 0..al/4: where the reference's comparison and the variant's differ."""
    al = np.repeat(np.arange(50, 301), 76)
    ed = np.tile(np.arange(76), 251)
    ok = ed <= al // 4
    al, ed = al[ok], ed[ok]
    v = identity_variants(al, ed, f32(thr))
    return {k: list(zip(al[v["ref"] != v[k]].tolist(), ed[v["ref"] != v[k]].tolist())) for k in ("gt", "f64")}


@functools.lru_cache(maxsize=None)
def percent_ties(thr):
    """{variant: [(al, l_seq)]} over l_seq 50..301, al 1..l_seq."""
    ls = np.repeat(np.arange(50, 302), 301)
    al = np.tile(np.arange(1, 302), 252)
    ok = al <= ls
    al, ls = al[ok], ls[ok]
    v = percent_variants(al, ls, f32(thr))
    return {k: list(zip(al[v["ref"] != v[k]].tolist(), ls[v["ref"] != v[k]].tolist())) for k in ("gt", "f64", "recip")}


def identity_tie(thr, single):
    """Pairs (or, single, records) exactly where >= and >, f32 and f64 part, each with its neighbours one edit more and one fewer."""
    ties = identity_ties(thr)
    s = Sample()
    sets = {}
    k = 0
    s.fill(20)
    for variant in ("gt", "f64"):
        sets[variant] = []
        for al, ed0 in spread(ties[variant]):
            for ed in (ed0 - 1, ed0, ed0 + 1):
                if ed < 0:
                    continue
                keep = bool(identity_variants([al], [ed], f32(thr))["ref"][0])
                name = s.lname(b"t%d" % int(thr * 100), k)
                if single:      # the record under test carries two deleted bases, which count for a single read (filter.rs:256-263); its mate is spotless
                    me, mate = dict(cigar="%dM2D%dM" % (al - 2 - al // 3, al // 3), nm=ed), dict()
                    i1, i2 = s.pair(name, keep, *((me, mate) if k % 2 else (mate, me)))
                else:           # the pair's sums, split unevenly
                    a1, e1 = al // 3, ed // 3
                    i1, i2 = s.pair(name, keep, dict(cigar="%dM" % a1, nm=e1), dict(cigar="%dM" % (al - a1), nm=ed - e1))
                sets[variant].append(dict(al=al, ed=ed, tie=ed == ed0, keep=keep, records=(i1, i2)))
                k += 1
                s.fill(2)
    s.fill(20)
    fp = params(min_percent_identity_single=thr, min_aligned_length_pair=1) if single else params(min_percent_identity_pair=thr)
    return s.case("identity_tie_%s_%d" % ("single" if single else "pair", round(thr * 100)), "judge", fp, meta=dict(thr=float(f32(thr)), sets=sets))


def percent_tie(thr, single):
    ties = percent_ties(thr)
    s = Sample()
    sets = {}
    k = 0
    s.fill(20)
    for variant in ("gt", "f64", "recip"):
        sets[variant] = []
        for al0, ls in spread(ties[variant]):
            for al in (al0 - 1, al0, al0 + 1):
                if al > ls:
                    continue
                keep = bool(percent_variants([al], [ls], f32(thr))["ref"][0])
                name = s.lname(b"a%d" % int(thr * 100), k)
                if single:      # two deleted bases count as aligned for a single read
                    me, mate = dict(cigar="%dM2D%dM%dS" % (al - 2 - al // 3, al // 3, ls - (al - 2))), dict()
                    i1, i2 = s.pair(name, keep, *((me, mate) if k % 2 else (mate, me)))
                else:           # the denominator is the sum of both l_seq: a third and two thirds
                    l1 = ls // 3
                    a1 = max(min(al // 3, l1), al - (ls - l1))
                    i1, i2 = s.pair(name, keep, dict(cigar="%dM%dS" % (a1, l1 - a1) if l1 > a1 else "%dM" % a1),
                                    dict(cigar="%dM%dS" % (al - a1, ls - l1 - (al - a1)) if ls - l1 > al - a1 else "%dM" % (al - a1)))
                sets[variant].append(dict(al=al, ls=ls, tie=al == al0, keep=keep, records=(i1, i2)))
                k += 1
                s.fill(2)
    s.fill(20)
    fp = params(min_aligned_percent_single=thr, min_aligned_length_pair=1) if single else params(min_aligned_percent_pair=thr)
    return s.case("percent_tie_%s_%d" % ("single" if single else "pair", round(thr * 100)), "judge", fp, meta=dict(thr=float(f32(thr)), sets=sets))


def aligned_length(single):
    """At the bound, one below, deletions (which count for a single read and not for a pair), = and X (which count), N S H P (which do not)."""
    s = Sample()
    s.fill(15)
    rows = [("100M", True), ("99M", False), ("90M10D", single), ("100=", True), ("100X", True), ("40=30X30M", True), ("99=", False), ("99X", False),
            ("50M50N", False), ("50M50S", False), ("50M50H", False), ("50M50P", False), ("50M50N50M", True), ("50M49N1D50M", True)]
    claims = []
    for k, (c, keep) in enumerate(rows):
        name = s.lname(b"L", k)
        me, mate = dict(cigar=c), dict()
        i1, i2 = s.pair(name, keep, *((me, mate) if k % 2 else (mate, me)))
        claims.append(dict(cigar=c, keep=keep, records=(i1, i2)))
        s.fill(3)
    s.fill(15)
    # the mate brings 100 aligned bases: the pair's bound of 200 asks the record under test for 100, as the single bound does directly
    fp = params(min_aligned_length_single=100, min_aligned_length_pair=1) if single else params(min_aligned_length_pair=200)
    return s.case("aligned_length_%s" % ("single" if single else "pair"), "judge", fp, meta=dict(claims=claims))


MAPQ_MATES = ((29, 30), (30, 29), (30, 30), (255, 30), (30, 255), (0, 0), (60, 60))


def mapq(min_mapq, single):
    """min_mapq 0: only MAPQ 255 is excluded; 30: 29 and 255 are; 255: nothing is (filter.rs:250-254, :289-296)."""
    s = Sample()
    s.fill(10)
    claims = []
    for k, (m1, m2) in enumerate(MAPQ_MATES):
        keep = min_mapq == 255 or (min(m1, m2) >= min_mapq and 255 not in (m1, m2))
        i1, i2 = s.pair(s.lname(b"q%d" % min_mapq, k), keep, dict(mapq=m1), dict(mapq=m2))
        claims.append(dict(mapq=(m1, m2), keep=keep, records=(i1, i2)))
        s.fill(2)
    s.rec(b"lone", mapq=255)                                     # parked and never taken out, whatever the bound
    s.fill(10)
    fp = params(min_mapq=min_mapq, min_aligned_length_pair=1, **(dict(min_aligned_length_single=1) if single else {}))
    return s.case("mapq_%d_%s" % (min_mapq, "single" if single else "pair"), "judge", fp, meta=dict(claims=claims))


def zero_lengths(kind):
    """l_seq == 0 and aligned length 0: the reference divides, and compares what comes out (inf, -inf, NaN) with >=."""
    s = Sample()
    s.fill(10)
    zs = dict(cigar="50S50N")                                    # aligned 0, l_seq 50
    rows = {
        # aligned percent and identity bounds of 0.5 on the pair
        "pair": [("one l_seq 0", dict(l_seq=0), {}, True),                          # 200 / 100
                 ("both l_seq 0", dict(l_seq=0), dict(l_seq=0), True),              # 200 / 0 = inf
                 ("aligned 0, NM 0", zs, zs, False),                                # 0 / 100 < 0.5
                 ("aligned 0, NM 1", dict(zs, nm=1), zs, False),
                 ("aligned 0 and l_seq 0", dict(cigar="50N"), dict(cigar="50N"), False),      # 0 / 0 = NaN
                 ("one aligned 0", zs, {}, True)],                                  # 100 / 150, identity 1
        # every threshold 0 (a MAPQ bound with proper pairs only, filter.rs:48-61: the single-read predicate runs as well): NaN >= 0 and
        # -inf >= 0 are false
        "thr0": [("one l_seq 0", dict(l_seq=0), {}, True),
                 ("both l_seq 0", dict(l_seq=0), dict(l_seq=0), True),
                 ("aligned 0, NM 0", zs, zs, False),                                # 1 - 0 / 0 = NaN
                 ("aligned 0, NM 1", zs, dict(zs, nm=1), False),                    # 1 - 1 / 0 = -inf
                 ("aligned 0 and l_seq 0", dict(cigar="50N"), dict(cigar="50N"), False),
                 ("one aligned 0", {}, zs, False)],                                 # the pair's sums would pass, the read's own identity is NaN
        # identity bound of 0.5 on the pair alone: the aligned percent (0 / 100, NaN) passes its bound of 0
        "pair_identity": [("both l_seq 0", dict(l_seq=0), dict(l_seq=0), True),
                          ("aligned 0, NM 0", zs, zs, False),                       # NaN
                          ("aligned 0, NM 1", dict(zs, nm=1), zs, False),           # -inf
                          ("aligned 0 and l_seq 0", dict(cigar="50N"), dict(cigar="50N"), False)],
        # aligned percent bound of 0.5 on each read
        "single_percent": [("l_seq 0", dict(l_seq=0), {}, True),                    # 100 / 0 = inf
                           ("aligned 0", {}, zs, False),                            # 0 / 50
                           ("aligned 0 and l_seq 0", dict(cigar="50N"), {}, False)],
        # identity bound of 0.5 on each read
        "single_identity": [("l_seq 0", {}, dict(l_seq=0), True),
                            ("aligned 0, NM 0", zs, {}, False),                     # NaN
                            ("aligned 0, NM 1", {}, dict(zs, nm=1), False)],        # -inf
    }[kind]
    claims = []
    for k, (what, a, b, keep) in enumerate(rows):
        i1, i2 = s.pair(s.lname(b"z", k), keep, a, b)
        claims.append(dict(what=what, keep=keep, records=(i1, i2)))
        s.fill(2)
    s.fill(10)
    fp = {"pair": lambda: params(min_aligned_percent_pair=0.5, min_percent_identity_pair=0.5),
          "thr0": lambda: params(proper=True, min_mapq=30),
          "pair_identity": lambda: params(min_percent_identity_pair=0.5),
          "single_percent": lambda: params(min_aligned_percent_single=0.5, min_aligned_length_pair=1),
          "single_identity": lambda: params(min_percent_identity_single=0.5, min_aligned_length_pair=1)}[kind]()
    return s.case("zero_lengths_%s" % kind, "judge", fp, meta=dict(claims=claims))


ZERO_KINDS = ("pair", "thr0", "pair_identity", "single_percent", "single_identity")


# ---------------------------------------------------------------------------------------------- judgement: the NM error
ABSENT, BAD = dict(nm_kind=bamio.NM_ABSENT), dict(nm_kind=bamio.NM_BADTYPE)


def nm_case(kind):
    s = Sample(2)
    s.fill(12)
    error = None
    fp = params(min_percent_identity_pair=0.9, min_mapq=30)
    if kind == "a_mapq_first":              # the pair fails on MAPQ before NM is asked for
        s.pair(s.lname(b"n", 0), False, dict(ABSENT, mapq=10), dict(ABSENT))
        s.fill(3)
        s.pair(s.lname(b"n", 1), False, dict(BAD), dict(BAD, mapq=255))
    elif kind == "a_single_mapq_255_first":     # filter_single: MAPQ 255 ends the single-read predicate before NM is asked for (filter.rs:250-254)
        fp = params(min_aligned_length_single=1, min_mapq=30, min_aligned_length_pair=1)
        s.pair(s.lname(b"n", 0), False, dict(ABSENT, mapq=255), dict(ABSENT))
        s.fill(3)
        s.pair(s.lname(b"n", 1), False, {}, dict(BAD, mapq=255))
    elif kind == "b_single_first_fails":    # filter_single: the first record fails its percent bound, the second is not looked at
        fp = params(min_aligned_percent_single=0.9, min_aligned_length_pair=1)
        s.pair(s.lname(b"n", 0), False, dict(cigar="50M50S"), dict(ABSENT))
        s.fill(3)
        s.pair(s.lname(b"n", 1), False, dict(cigar="50M50S"), dict(BAD))
    elif kind in ("c_bad_then_absent", "c_absent_then_bad"):
        first, second = (BAD, ABSENT) if kind == "c_bad_then_absent" else (ABSENT, BAD)
        s.pair(s.lname(b"n", 0), False, {}, dict(first))
        s.fill(3)
        s.pair(s.lname(b"n", 1), False, dict(second), {})
        error = 3 if first is BAD else 2
    elif kind == "c_both_in_one_pair":      # the second record's NM is asked for first (filter.rs:298-299: record, then record1)
        s.pair(s.lname(b"n", 0), False, dict(BAD), dict(ABSENT))
        error = 2
    elif kind == "c_single_asks_the_first_record_first":      # filter_single: the first record's predicate runs first (filter.rs:190-203)
        fp = params(min_percent_identity_single=0.5, min_aligned_length_pair=1)
        s.pair(s.lname(b"n", 0), False, dict(BAD), dict(ABSENT))
        error = 3
    elif kind == "d_never_judged":
        s.rec(b"lone", **ABSENT)                                      # parked, never taken out
        s.rec(b"away", mtid=1, **BAD)                                 # mate elsewhere: not parked
        s.pair(b"sec", False, dict(ABSENT, flag=99 | 0x100), dict(ABSENT, flag=147 | 0x100))
        s.pair(b"sup", False, dict(BAD, flag=99 | 0x800), dict(BAD, flag=147 | 0x800))
        s.pair(b"imp", False, dict(ABSENT, flag=97), dict(ABSENT, flag=145))
    elif kind in ("e_list_then_entry", "e_entry_then_list"):
        def triple(fault):                  # A B C of one name, all parking: A and B are judged from the list, C is left
            a = s.rec(b"tri")
            s.fill(1)
            s.rec(b"tri", flag=147, **fault)
            s.fill(1)
            s.rec(b"tri")
            return a
        if kind == "e_list_then_entry":
            triple(ABSENT)
            s.fill(2)
            s.pair(s.lname(b"n", 0), False, {}, dict(BAD))
            error = 2
        else:
            s.pair(s.lname(b"n", 0), False, {}, dict(BAD))
            s.fill(2)
            triple(ABSENT)
            error = 3
    else:
        raise KeyError(kind)
    s.fill(12)
    return s.case("nm_" + kind, "nm", fp, error=error)


NM_KINDS = ("a_mapq_first", "a_single_mapq_255_first", "b_single_first_fails", "c_bad_then_absent", "c_absent_then_bad", "c_both_in_one_pair", "c_single_asks_the_first_record_first",
            "d_never_judged", "e_list_then_entry", "e_entry_then_list")


# ---------------------------------------------------------------------------------------------- parking (filter.rs:163-187)
def parking(kind):
    """Record by record; "here" = the mate's reference is the record's own, "away" = another one."""
    s = Sample(3)
    away = dict(mtid=2)
    s.fill(8)
    F = lambda: s.fill(2)
    if kind == "first_away":                # A (away) B (here): A is not parked, B is parked and waits for ever
        s.rec(b"x", **away); F(); s.rec(b"x", flag=147)
    elif kind == "second_away":             # A (here) B (away): A is parked, B takes it out whatever its own mate reference says
        a = s.rec(b"x"); F(); b = s.rec(b"x", flag=147, **away); s.keep(a, b)
    elif kind == "abc_first_not_parking":   # A (away) B (here) C (here): B and C
        s.rec(b"x", **away); F(); b = s.rec(b"x", flag=147); F(); c = s.rec(b"x"); s.keep(b, c)
    elif kind == "abc_all_parking":         # A B C (here): A and B, C is parked and left
        a = s.rec(b"x"); F(); b = s.rec(b"x", flag=147); F(); s.rec(b"x"); s.keep(a, b)
    elif kind == "abcd":                    # two pairs, in the order of B and D, other pairs' second records between them
        a = s.rec(b"x"); y1 = s.rec(b"y"); b = s.rec(b"x", flag=147); F(); y2 = s.rec(b"y", flag=147); c = s.rec(b"x"); F(); d = s.rec(b"x", flag=147)
        s.keep(a, b); s.keep(y1, y2); s.keep(c, d)
    elif kind == "abcd_middle_away":        # A (here) B (away) C (away) D (here): A and B; C is not parked, D is parked and left
        a = s.rec(b"x"); F(); b = s.rec(b"x", flag=147, **away); F(); s.rec(b"x", **away); F(); s.rec(b"x", flag=147); s.keep(a, b)
    elif kind == "five":                    # (1, 2), (3, 4), the fifth is left
        i = []
        for k in range(5):
            i.append(s.rec(b"x", flag=147 if k % 2 else 99)); F()
        s.keep(i[0], i[1]); s.keep(i[2], i[3])
    elif kind == "five_second_away":        # 1 (here) 2 (away: taken) 3 (away: not parked) 4 (here: parked) 5 (here: takes 4)
        i = []
        for k in range(5):
            i.append(s.rec(b"x", flag=147 if k % 2 else 99, **(away if k in (1, 2) else {}))); F()
        s.keep(i[0], i[1]); s.keep(i[3], i[4])
    elif kind == "two_references":          # the set is emptied at a reference change (filter.rs:149-161): no pair across
        s.rec(b"x"); F(); s.rec(b"y"); s.fill(3, tid=1)
        s.rec(b"x", tid=1, flag=147); a = s.rec(b"y", tid=1); s.fill(2, tid=1); b = s.rec(b"y", tid=1, flag=147); s.keep(a, b)
        s.rec(b"x", tid=2, mtid=1); s.fill(2, tid=2)
    elif kind == "secondary_and_improper":  # only the two primary proper-pair records of the name take part
        s.rec(b"x", flag=99 | 0x100); s.rec(b"x", flag=97); a = s.rec(b"x"); F(); s.rec(b"x", flag=147 | 0x800); s.rec(b"x", flag=145)
        b = s.rec(b"x", flag=147); s.rec(b"x", flag=99 | 0x100); s.keep(a, b)
    elif kind == "unmapped_flag_with_proper":     # 0x4 beside 0x2: the reference lets such a record fall through to the pairing
        a = s.rec(b"x", flag=99 | 0x4); F(); b = s.rec(b"x", flag=147); s.keep(a, b)
        c = s.rec(b"y"); d = s.rec(b"y", flag=147 | 0x4); s.keep(c, d)
        s.rec(b"u", flag=0x4 | 0x1 | 0x40); s.rec(b"u", flag=0x4 | 0x1 | 0x80)
    else:
        raise KeyError(kind)
    # the last reference a record can lie on keeps the order rule of Sample.rec
    last = max(r[1] for r in s.rows)
    s.rec(b"alone", tid=last)                                    # parked and never taken out
    s.fill(8, tid=last)
    return s.case("parking_" + kind, "park", params(min_percent_identity_pair=0.9))


PARKING_KINDS = ("first_away", "second_away", "abc_first_not_parking", "abc_all_parking", "abcd", "abcd_middle_away", "five", "five_second_away", "two_references",
                 "secondary_and_improper", "unmapped_flag_with_proper")


# ---------------------------------------------------------------------------------------------- output order across the scan's block of 4 096 records
def output_order():
    """Nested (A1 B1 B2 A2) and interleaved (A1 B1 A2 B2) pairs from record 0 to beyond the scan block's border at 4 096; every fifth group
    loses one of its pairs to the identity bound, CIGARs of one to four words."""
    s = Sample()
    cig = ("100M", "60M2I38M", "30M1D30M1I39M", "20M1I20M1D20M1I38M")
    g = 0
    crossed = False
    while len(s.rows) < 4096 + 200:
        if not crossed and len(s.rows) >= 4080:                   # six pairs whose records lie on both sides of the border: three nested, three interleaved
            crossed = True
            while len(s.rows) < 4090:
                s.rec(b"lone.%d" % len(s.rows))
            first = [s.rec(b"X%d" % k, cigar=cig[k % 4]) for k in range(6)]
            assert len(s.rows) == 4096
            for k in (2, 1, 0, 3, 4, 5):
                s.keep(first[k], s.rec(b"X%d" % k, flag=147, cigar=cig[(k + 1) % 4]))
        a, b = b"A%d" % g, b"B%d" % g
        bad = dict(nm=30) if g % 5 == 0 else {}
        ca, cb = dict(cigar=cig[g % 4]), dict(cigar=cig[(g // 4 + 1) % 4])
        if len(s.rows) % 3 == 2 and g % 2:
            s.rec(b"lone%d" % g)                                  # shifts the groups against the border
        a1 = s.rec(a, **ca)
        b1 = s.rec(b, **dict(cb, **bad))
        if g % 2:
            b2 = s.rec(b, flag=147, **cb); a2 = s.rec(a, flag=147, **ca)
        else:
            a2 = s.rec(a, flag=147, **ca); b2 = s.rec(b, flag=147, **cb)
        s.keep(a1, a2)
        if not bad:
            s.keep(b1, b2)
        g += 1
    return s.case("output_order", "order", params(min_percent_identity_pair=0.9))


# ---------------------------------------------------------------------------------------------- the join table, keys injected with cov_set_mates
def _with_keys(s, id, over, group="table", **kw):
    """over: {record index: (qh1, qh2)}; every other record keeps the hash of its name."""
    b = s.bam()
    hs = [_hash(n) for n in b.qname]
    qh1 = np.asarray([over[i][0] if i in over else h[0] for i, h in enumerate(hs)], np.uint64)
    qh2 = np.asarray([over[i][1] if i in over else h[1] for i, h in enumerate(hs)], np.uint32)
    return Case(id, group, b, params(min_percent_identity_pair=0.9), s.order(), None, keys=(qh1, qh2), **kw)


def _key_at(rng, want, tid, mask, qh1=None):
    """A random key (qh1 given or drawn) whose probe run starts at a slot `want` accepts."""
    while True:
        a = int(rng.integers(2, 1 << 63)) if qh1 is None else qh1
        c = int(rng.integers(0, 1 << 32))
        if want(slot_of(a, c, tid, mask)):
            return a, c


def table_zero_and_one():
    """qh1 == 0 is stored as 1: with equal qh2 the two are one name (by design), with different qh2 two names."""
    s = Sample()
    over = {}
    s.fill(10)
    a = s.rec(b"p"); s.fill(1); b = s.rec(b"q", flag=147); s.keep(a, b)
    over[a], over[b] = (0, 7), (1, 7)
    s.fill(2)
    c = s.rec(b"r"); d = s.rec(b"s"); s.fill(1); e = s.rec(b"t", flag=147); f = s.rec(b"u", flag=147)
    over[c], over[d], over[e], over[f] = (0, 8), (1, 9), (1, 8), (0, 9)
    s.keep(c, e); s.keep(d, f)
    s.fill(2)
    g = s.rec(b"v"); h = s.rec(b"w", flag=147)                   # 0 | 11 and 1 | 12: two names, each alone
    over[g], over[h] = (0, 11), (1, 12)
    s.fill(10)
    return _with_keys(s, "table_zero_and_one", over)


def table_equal_first_word():
    """Two keys with one qh1, different qh2 and one starting slot, two records each, then the same with three and two records: they stay
    entries of their own."""
    rng = np.random.default_rng(11)
    s = Sample()
    over = {}
    s.fill(10)
    for n_first in (2, 3):
        q1 = int(rng.integers(2, 1 << 63))
        _, c1 = _key_at(rng, lambda x: True, 0, 1023, q1)
        slot = slot_of(q1, c1, 0, 1023)
        _, c2 = _key_at(rng, lambda x: x == slot, 0, 1023, q1)
        assert c1 != c2
        a1 = s.rec(b"e1"); b1 = s.rec(b"e2"); s.fill(1); b2 = s.rec(b"e2", flag=147); a2 = s.rec(b"e1", flag=147)
        over.update({a1: (q1, c1), a2: (q1, c1), b1: (q1, c2), b2: (q1, c2)})
        s.keep(a1, a2); s.keep(b1, b2)
        if n_first == 3:
            s.fill(1)
            over[s.rec(b"e1")] = (q1, c1)                       # a third record of the first key: parked and left
        s.fill(2)
    s.fill(10)
    return _with_keys(s, "table_equal_first_word", over, meta=dict(over=over))


def table_equal_key_other_reference():
    s = Sample(2)
    over = {}
    key = (0x1234567890ABCDEF, 0xCAFE)
    s.fill(8)
    over[s.rec(b"k")] = key                                      # alone on reference 0
    s.fill(8)
    s.fill(4, tid=1)
    a = s.rec(b"k", tid=1, flag=147); s.fill(2, tid=1); b = s.rec(b"k", tid=1); s.keep(a, b)
    over[a] = over[b] = key
    s.fill(4, tid=1)
    return _with_keys(s, "table_equal_key_other_reference", over)


def table_wrap(n_records, injected=True):
    """40 names whose probe runs start in the last three slots of the table of a chunk of n_records records (1 024 entries for 512 records,
    2 048 for 513): every run wraps past the last slot.  One of the names has three records, so that k_pair_collect walks the same run."""
    size = table_size(n_records)
    mask = size - 1
    rng = np.random.default_rng(n_records)
    s = Sample()
    over = {}
    last3 = lambda x: x >= size - 3
    keys = []
    taken = set()
    for k in range(40):
        if injected:
            keys.append((b"w%d" % k, _key_at(rng, last3, 0, mask)))
        else:
            n = name_with(b"w", last3, 0, mask, taken)
            taken.add(n)
            keys.append((n, None))
    n_fill = (n_records - 81) // 2
    s.fill(n_fill // 2)
    firsts = []
    for k, (n, key) in enumerate(keys):
        i = s.rec(n)
        firsts.append(i)
        over[i] = key
    for k, (n, key) in reversed(list(enumerate(keys))):
        i = s.rec(n, flag=147)
        over[i] = key
        s.keep(firsts[k], i)
    i = s.rec(keys[17][0])                                       # the third record of one name: parked and left
    over[i] = keys[17][1]
    s.fill(n_fill - n_fill // 2)
    while len(s.rows) < n_records:
        s.rec(b"pad%d" % len(s.rows))
    assert len(s.rows) == n_records
    id = "table_wrap_%d_%s" % (n_records, "keys" if injected else "names")
    meta = dict(size=size, names=[n for n, _ in keys])
    if injected:
        return _with_keys(s, id, over, meta=meta)
    return s.case(id, "table", params(min_percent_identity_pair=0.9), meta=meta)


# ---------------------------------------------------------------------------------------------- chunk cuts (pair_chunk = 1024)
def _reference(s, tid, n, tag, triple=False):
    """n records on reference tid: pairs whose mates lie 1 .. 40 records apart, one name of three records if asked."""
    start = len(s.rows)
    if triple:
        s.rec(b"%s.tri" % tag, tid)
    pending = []
    k = 0
    while len(s.rows) - start + len(pending) < n - (2 if triple else 0) - 1:
        name = b"%s.%d" % (tag, k)
        pending.append((s.rec(name, tid, nm=30 if k % 9 == 0 else 0), name, k))
        if len(pending) > k % 20:
            i1, nm_, kk = pending.pop(0)
            i2 = s.rec(nm_, tid, flag=147)
            if kk % 9:
                s.keep(i1, i2)
        k += 1
    for i1, nm_, kk in pending:
        i2 = s.rec(nm_, tid, flag=147)
        if kk % 9:
            s.keep(i1, i2)
    if triple:
        a = start
        b = s.rec(b"%s.tri" % tag, tid, flag=147)
        s.keep(a, b)
        s.rec(b"%s.tri" % tag, tid)
    while len(s.rows) - start < n:
        s.rec(b"%s.pad%d" % (tag, len(s.rows)), tid)
    assert len(s.rows) - start == n, (len(s.rows) - start, n)


def chunks(kind):
    sizes, triples, tail = {
        "exactly_1024_then_others": ((1024, 300, 301), (), 0),
        "1023_and_1025": ((1023, 1025), (), 0),
        "3500_two_empty_chunks": ((3500, 100), (), 0),
        "no_reference_at_the_end": ((700, 324), (), 30),
        "triples_in_first_middle_last": ((1030, 1024, 1100, 500), (0, 2, 3), 0),
    }[kind]
    s = Sample(len(sizes))
    for t, n in enumerate(sizes):
        _reference(s, t, n, b"c%d" % t, t in triples)
    if tail:      # records without a reference: two proper-pair names among them (mate reference -1 as well), the rest ordinary unmapped mates
        a = s.rec(b"un1", -1, flag=99 | 0x4)
        for k in range(tail - 4):
            s.rec(b"u%d" % (k // 2), -1, flag=(77, 141)[k % 2], cigar="", l_seq=100, nm_kind=bamio.NM_ABSENT)
        b = s.rec(b"un1", -1, flag=147 | 0x4)
        s.keep(a, b)
        s.rec(b"un2", -1, flag=99 | 0x4, mtid=0)
        s.rec(b"un2", -1, flag=147 | 0x4)
    return s.case("chunks_" + kind, "chunk", params(min_percent_identity_pair=0.9), knobs=dict(pair_chunk=1024), meta=dict(sizes=sizes))


CHUNK_KINDS = ("exactly_1024_then_others", "1023_and_1025", "3500_two_empty_chunks", "no_reference_at_the_end", "triples_in_first_middle_last")


# ---------------------------------------------------------------------------------------------- the list cap (pair_multi_cap = 64)
def list_cap(over):
    """Names of three records: 20 and one of four list 64 records, which the device takes; 22 list 66, which it declines."""
    s = Sample()
    s.fill(10)
    n3 = 22 if over else 20
    first = {}
    for k in range(n3):
        first[k] = s.rec(b"m%d" % k)
    s.fill(5)
    for k in range(n3):
        s.keep(first[k], s.rec(b"m%d" % k, flag=147))
    for k in range(n3):
        s.rec(b"m%d" % k)
    if not over:
        i = [s.rec(b"four", flag=147 if k % 2 else 99) for k in range(4)]
        s.keep(i[0], i[1]); s.keep(i[2], i[3])
    s.fill(10)
    listed = 3 * n3 + (0 if over else 4)
    return s.case("list_cap_%d" % listed, "cap", params(min_percent_identity_pair=0.9), knobs=dict(pair_multi_cap=64), declined=over, meta=dict(listed=listed))


def list_cap_floor(over):
    """pair_multi_cap = 1 is taken as 16, the knob's floor: four names of four records list 16, which the device takes; a name of three
    more makes 19, which it declines.  (Were the value ignored, neither would be declined; were it taken as 1, both would.)"""
    s = Sample()
    s.fill(10)
    for k in range(4):
        i = [s.rec(b"four%d" % k, flag=147 if j % 2 else 99) for j in range(4)]
        s.keep(i[0], i[1]); s.keep(i[2], i[3])
        s.fill(1)
    if over:
        a = s.rec(b"three"); b = s.rec(b"three", flag=147); s.rec(b"three")
        s.keep(a, b)
    s.rec(b"alone")
    s.fill(10)
    listed = 19 if over else 16
    return s.case("list_cap_floor_%d" % listed, "cap", params(min_percent_identity_pair=0.9), knobs=dict(pair_multi_cap=1), declined=over, meta=dict(listed=listed))


# ---------------------------------------------------------------------------------------------- all of them
@functools.lru_cache(maxsize=None)
def all_cases():
    out = []
    for single in (False, True):
        out += [identity_tie(t, single) for t in IDENTITY_THRESHOLDS]
        out += [percent_tie(t, single) for t in PERCENT_THRESHOLDS]
        out.append(aligned_length(single))
        out += [mapq(m, single) for m in (0, 30, 255)]
    out += [zero_lengths(k) for k in ZERO_KINDS]
    out += [nm_case(k) for k in NM_KINDS]
    out += [parking(k) for k in PARKING_KINDS]
    out.append(output_order())
    out += [table_zero_and_one(), table_equal_first_word(), table_equal_key_other_reference()]
    out += [table_wrap(n, inj) for n in (512, 513) for inj in (True, False)]
    out += [chunks(k) for k in CHUNK_KINDS]
    out += [list_cap(False), list_cap(True), list_cap_floor(False), list_cap_floor(True)]
    assert len({c.id for c in out}) == len(out)
    return tuple(out)


def case(id):
    return next(c for c in all_cases() if c.id == id)


def concatenated(cases):
    """The cases' samples as one sample, one run of references per case (a case's own references stay apart).  Returns the BamData and, per
    case, the offset of its records."""
    names, tid, mtid, parts, offs = [], [], [], [], []
    at = 0
    for k, c in enumerate(cases):
        b = c.bam
        base = len(names)
        names += ["k%d_%s" % (k, n) for n in b.ref_names]
        assert (b.tid >= 0).all()
        tid.append(b.tid + base)
        mtid.append(np.where(b.mtid >= 0, b.mtid + base, b.mtid))
        parts.append(b)
        offs.append(at)
        at += b.n_records
    cat = lambda f, dt: np.concatenate([np.asarray(getattr(b, f)) for b in parts]).astype(dt)
    ncig = np.concatenate([np.diff(b.cigar_off.astype(np.int64)) for b in parts])
    coff = np.zeros(at + 1, np.uint32)
    np.cumsum(ncig, out=coff[1:])
    z = np.zeros(at, np.int32)
    bam = bamio.BamData(names, np.full(len(names), parts[0].ref_lens[0], np.int64), np.concatenate(tid).astype(np.int32), (100 + 10 * np.arange(at)).astype(np.int32),
                        cat("flag", np.uint16), cat("mapq", np.uint8), cat("l_seq", np.int32), cat("nm", np.uint32), cat("nm_kind", np.uint8), coff,
                        cat("cigar", np.uint32), np.concatenate(mtid).astype(np.int32), z.copy(), z.copy(), [q for b in parts for q in b.qname], "")
    return bam, offs
