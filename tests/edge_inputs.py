"""Inputs built to land on the decision points of the estimator kernels (k_estimate*, k_genome_estimate*: the trimmed mean's two indices,
the 64-bin batches of its walk, EST_SERIAL_BINS, the end exclusion) and of the exact parallel identity sums (k_id_*: binade crossings,
rounding ties, the borders of the 1024-record chunks).  Nothing here is left to chance: a staircase contig has exactly the window
histogram asked for, an identity chain exactly the values asked for at exactly the record indices asked for.  tests/test_edge_inputs.py
proves on the CPU, against the oracle and plain Python floats, that every case has the property it is named for; the GPU tests
(test_gpu_estimator_edges.py, test_gpu_identity_edges.py) then compare the device with the oracle on them.  Plain Python and numpy: no
code of the device is imported."""
import functools
import math
import struct
from fractions import Fraction

import numpy as np

from oracle.bamio import BamData

ID_CH = 1024            # records per chunk of the identity kernels (pileup_kernels.hip.h) — restated, the CPU test does not load the device's code
FILLER_ALIGNED = 100    # the non-dyadic filler records: 100M with NM 1 .. 7


# ------------------------------------------------------------------------------------------------ records
def records(names, lens, tid, pos, aligned, nm, flag=None) -> BamData:
    """Records `aligned M` with NM = nm, in the order given (it must be sorted by tid, then pos)."""
    n = len(tid)
    aligned = np.asarray(aligned, np.int64)
    z = np.zeros(n, np.int32)
    return BamData(list(names), np.asarray(lens, np.int64), np.asarray(tid, np.int32), np.asarray(pos, np.int32),
                   np.zeros(n, np.uint16) if flag is None else np.asarray(flag, np.uint16), np.full(n, 60, np.uint8), aligned.astype(np.int32),
                   np.asarray(nm, np.uint32), np.ones(n, np.uint8), np.arange(n + 1, dtype=np.uint32), (aligned << 4).astype(np.uint32), z, z, z, [], "")


def concat(parts) -> BamData:
    """The contigs of `parts` back to back in one sample, their records in the same order."""
    names, lens, cols, base = [], [], [], 0
    for k, b in enumerate(parts):
        names += ["p%d_%s" % (k, n) for n in b.ref_names]
        lens += [int(x) for x in b.ref_lens]
        cols.append((b.tid.astype(np.int64) + base, b.pos, b.l_seq, b.nm, b.flag))
        base += len(b.ref_names)
    cat = [np.concatenate([c[j] for c in cols]) for j in range(5)]
    return records(names, lens, cat[0], cat[1], cat[2], cat[3], cat[4])


def bare(length) -> BamData:
    """A contig without a record."""
    return records(["bare"], [length], [], [], [], [])


def short_with_reads(length=149) -> BamData:
    """A contig shorter than twice an end exclusion of 75, with two reads."""
    return records(["short"], [length], [0, 0], [0, 3], [length, length - 5], [1, 0])


def as_counts(counts) -> dict:
    """{depth: bases} of a list (index = depth) or a dict; empty bins dropped, bin 0 kept."""
    items = counts.items() if isinstance(counts, dict) else enumerate(counts)
    c = {int(d): int(n) for d, n in items if n > 0 or d == 0}
    c.setdefault(0, 0)
    assert all(d >= 0 and n >= 0 for d, n in c.items())
    return c


def dense(counts, n_bins=None) -> np.ndarray:
    c = as_counts(counts)
    out = np.zeros(max(max(c) + 1, n_bins or 0), np.uint64)
    for d, n in c.items():
        out[d] = n
    return out


def staircase(counts, excl=0, pad_left=0, pad_right=None, mid=0, mid_after=None, cut_left=0, nm=0) -> BamData:
    """One contig whose window [excl, length - excl) has exactly the depth histogram `counts` (a list, or the sparse form {depth: bases}:
    depth 599 costs 599 records).  For every depth d >= 1 with counts[d] > 0 one segment of counts[d] bases under d identical records
    `counts[d]M`, the segments disjoint and ascending in depth and position.  The counts[0] uncovered window bases: `pad_left` in front of
    the first segment, `mid` behind the segment of depth `mid_after`, the rest (`pad_right`, if given it must be the rest) behind the last.
    The 2 x excl border bases are uncovered, except that the records of the first segment start `cut_left` bases inside the left border
    (the window's border then cuts through them; pad_left must be 0)."""
    c = as_counts(counts)
    rest = c[0] - pad_left - mid
    assert rest >= 0 and (pad_right is None or pad_right == rest), (c[0], pad_left, mid, pad_right)
    assert cut_left <= excl and (cut_left == 0 or pad_left == 0)
    depths = sorted(d for d in c if d >= 1)
    assert mid == 0 or mid_after in depths
    pos, aligned, p = [], [], excl + pad_left
    for k, d in enumerate(depths):
        cut = cut_left if k == 0 else 0
        pos += [p - cut] * d
        aligned += [c[d] + cut] * d
        p += c[d]
        if d == mid_after:
            p += mid
    length = p + rest + excl
    n = len(pos)
    return records(["stair"], [length], np.zeros(n, np.int32), pos, aligned, np.minimum(nm, aligned) if n else [])


# ------------------------------------------------------------------------------------------------ the trimmed mean's indices
def f32_indices(T, trim_min, trim_max):
    """(min_index, max_index) as the reference takes them: floor(trim_min * T as f32), ceil(trim_max * T as f32), in f32."""
    t = np.float32(T)
    return int(np.floor(np.float32(trim_min) * t)), int(np.ceil(np.float32(trim_max) * t))


def prefix(counts):
    return np.cumsum(dense(counts).astype(np.int64))


def walk_points(counts, min_index, max_index):
    """(s, e) of the reference's loop over the inclusive prefix sums P: s = first bin with P >= min_index, e = first bin behind s with
    P > max_index — e == s when P[s] itself exceeds max_index (the reference's second branch), None where there is none."""
    P = prefix(counts)
    s = next((i for i in range(len(P)) if P[i] >= min_index), None)
    if s is None:
        return None, None
    if P[s] > max_index:
        return s, s
    return s, next((i for i in range(s + 1, len(P)) if P[i] > max_index), None)


def _spread(total, bins, heavy):
    """`total` bases over `bins`, one each and the rest on `heavy`."""
    bins = sorted(set(bins))
    assert total >= len(bins) and heavy in bins, (total, bins, heavy)
    out = {b: 1 for b in bins}
    out[heavy] += total - len(bins)
    return out


def trimmed_counts(T, trim, s, e, dv=0, ev=0, last=None, mids=(), empty0=False):
    """{depth: bases} with sum T whose prefix sums P stand in a stated relation to the two indices of `trim` at T:
        P[s-1] == min_index - 1 (s >= 1) and s is the first bin to reach min_index;
        e > s + 1:  P[s] == min_index + dv,  P[e-1] == max_index - ev,  P[e] > max_index;
        e == s + 1: P[s] == max_index - ev, P[e] > max_index;
        e == s:     P[s] == max_index + 1 (the first bin to reach min_index already exceeds max_index);
        e is None:  P[s] == min_index + dv and the last prefix, T, is <= max_index (no end bin).
    `last`: the highest occupied bin; `mids`: further bins to occupy (all others stay empty: runs of empty bins); `empty0`: bin 0 empty."""
    mn, mx = f32_indices(T, *trim)
    last = max(e if e is not None else s, s) + 1 if last is None else last
    mids = set(mids)
    c = {0: 0}
    if s >= 1:
        front = {m for m in mids if m < s} | {s - 1} | (set() if empty0 else {0}) | ({1} if s > 1 else set())
        c.update(_spread(mn - 1, front, min(front)))
        p_front = mn - 1
    else:
        p_front = 0
    if e is not None and e == s:
        c[s] = mx + 1 - p_front
        behind, total = {m for m in mids if m > s} | ({last} if last > s else set()), T - (mx + 1)
        if behind:
            c.update(_spread(total, behind, min(behind)))
        else:
            assert total == 0
    elif e is None:
        c[s] = mn + dv - p_front
        behind, total = {m for m in mids if m > s} | ({last} if last > s else set()), T - (mn + dv)
        assert T <= mx
        if behind:
            c.update(_spread(total, behind, max(behind)))
        else:
            assert total == 0
    else:
        assert e > s and last >= e
        between = {m for m in mids if s < m < e} | ({s + 1, e - 1} if e > s + 1 else set())
        if between:
            c[s] = mn + dv - p_front
            c.update(_spread(mx - ev - (mn + dv), between, e - 1))
        else:
            c[s] = mx - ev - p_front
        behind = {m for m in mids if e <= m <= last} | {e, last}
        c.update(_spread(T - (mx - ev), behind, e))
        assert c[e] >= ev + 1
    assert c[s] >= 0 and sum(c.values()) == T, (c, T)
    return c


# ------------------------------------------------------------------------------------------------ identity chains
def identity(aligned, nm) -> float:
    """One read's addend as the reference computes it (contig.rs:208-211)."""
    return (float(aligned) - float(nm)) / float(aligned)


def identity_chain(values, lead=0, flags=None) -> BamData:
    """Records `aligned M` with NM = nm for a list of (aligned, nm) pairs on one contig; `lead` filler records on a contig in front shift
    the first record's index in the sample.  `flags`: {index in values: SAM flag} for records that must not count."""
    parts = []
    for vals, fl in ((filler(lead), None), (values, flags)) if lead else ((values, flags),):
        n = len(vals)
        aligned = np.asarray([a for a, _ in vals], np.int64)
        nm = np.asarray([m for _, m in vals], np.int64)
        pos = np.arange(n) // 4
        flag = np.zeros(n, np.uint16)
        for i, f in (fl or {}).items():
            flag[i] = f
        parts.append(records(["chain"], [int(pos[-1] + aligned.max() + 1) if n else 1], np.zeros(n, np.int32), pos, aligned, nm, flag))
    return concat(parts) if len(parts) > 1 else parts[0]


def filler(n, start=0):
    """n non-dyadic filler records: 100M with NM 1 .. 7 in turn."""
    return [(FILLER_ALIGNED, 1 + (start + i) % 7) for i in range(n)]


ONE = (FILLER_ALIGNED, 0)        # identity 1.0
ZERO = (FILLER_ALIGNED, FILLER_ALIGNED)      # NM == aligned: identity 0.0, leaves the sum's bits alone


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def tie_at(x, e) -> bool:
    """frac(x / 2^(e-52)) == 1/2 exactly, from the bits of x: adding x to a sum in binade [2^e, 2^(e+1)) is an exact rounding tie."""
    b = _bits(x)
    ex = (b >> 52) & 0x7ff
    if ex == 0 or ex == 0x7ff:
        return False
    mant = (b & ((1 << 52) - 1)) | (1 << 52)
    sh = e - (ex - 1023)              # x / ulp = mant / 2^sh
    return sh >= 1 and (mant & ((1 << sh) - 1)) == 1 << (sh - 1)


@functools.lru_cache(maxsize=None)
def tie_pairs(e, max_aligned=1500):
    """Every (aligned, nm), 1 <= nm < aligned <= max_aligned, whose identity is a rounding tie in binade e (numpy on the same bits)."""
    a = np.arange(1, max_aligned + 1, dtype=np.float64)
    A, N = np.meshgrid(a, a, indexing="ij")
    keep = (N < A)
    A, N = A[keep], N[keep]
    b = ((A - N) / A).view(np.uint64)
    ex = ((b >> np.uint64(52)) & np.uint64(0x7ff)).astype(np.int64)
    mant = (b & np.uint64((1 << 52) - 1)) | np.uint64(1 << 52)
    sh = e - (ex - 1023)
    ok = (sh >= 1) & (sh <= 53) & (ex != 0)
    shc = np.clip(sh, 1, 53).astype(np.uint64)
    rem = mant & ((np.uint64(1) << shc) - np.uint64(1))
    ok &= rem == (np.uint64(1) << (shc - np.uint64(1)))
    return np.stack([A[ok].astype(np.int64), N[ok].astype(np.int64)], axis=1)


def wide_tie_pair(e):
    """A tie of binade e with aligned = 2^(e+2) + 1 (the binades no pair up to 1500 reaches)."""
    aligned = (1 << (e + 2)) + 1
    for nm in range(1, 4096):
        if tie_at(identity(aligned, nm), e):
            return aligned, nm
    raise AssertionError("no tie at binade %d" % e)


def tie_pair(e, k=0):
    """The k-th tie pair of binade e with an identity above 1/2."""
    if e >= 10:
        return wide_tie_pair(e)
    p = tie_pairs(e)
    p = p[2 * p[:, 1] < p[:, 0]]
    return tuple(int(x) for x in p[k % len(p)])


def binade(x) -> int:
    return math.frexp(x)[1] - 1


def replay(values, flip_ties=False, start=0.0):
    """The serial chain of rounded f64 additions over (aligned, nm) pairs in Python floats: (sums after each record, indices of the
    records that met the sum as an exact rounding tie).  flip_ties: every tie is rounded to the OTHER neighbour (away from half-even)."""
    S, sums, ties = start, [], []
    for i, (a, m) in enumerate(values):
        x = identity(a, m)
        r = S + x
        exact = Fraction(S) + Fraction(x)
        if Fraction(r) != exact:
            lo, hi = (math.nextafter(r, -math.inf), r) if Fraction(r) > exact else (r, math.nextafter(r, math.inf))
            if exact - Fraction(lo) == Fraction(hi) - exact:
                ties.append(i)
                if flip_ties:
                    r = lo if r == hi else hi
        S = r
        sums.append(S)
    return sums, ties


TIE_PLACES = ("chunk_first", "chunk_last", "lane0", "lane63", "head_lane0", "head_lane63", "tail")
TIE_BINADES = (1, 2, 5, 9, 10, 12)
AFTER = ID_CH + 40       # records behind the tie (but in a tail)


def _no_tie_filler(S, i):
    """The next filler (NM i, i + 1, ... mod 7) whose addition to S is no rounding tie: the chain's one tie is the record built for it."""
    for j in range(7):
        f = filler(1, i + j)[0]
        if not replay([f], start=S)[1]:
            return f
    raise AssertionError("every filler is a tie at %r" % S)


def tie_case(e, place, k=0):
    """(values, start, index of the tie record in values) of one tie case: the contig's first record must be record `start` (mod 1024) of
    the sample.  None where arithmetic rules the place out: addends <= 1 cannot lift the sum to binade e >= 10 inside a head of at most
    1023 records.
    Chain: [0.0 records (NM == aligned) where the place needs more records in front of the tie than the binade allows] + 2^e records of
    1.0 + 1 or 2 fillers (the sum is then inside binade e with low mantissa bits set) + the tie record + fillers while the sum stays at
    least 1.0 below the binade's end — from binade 10 on that is more than 1024 of them; below, where 1024 addends near 1 cannot fit
    into the binade, 0.0 records make up the number, so that the chunks behind the tie are whole and the contig ends in the binade."""
    core = [ONE] * (1 << e)
    for j in range(1 if e == 1 else 1 + k % 2):
        core.append(_no_tie_filler(replay(core)[0][-1], k + j))
    t = len(core)                                      # records in front of the tie, without padding
    if place.startswith("head"):
        start = 1                                      # the head: records 1 .. 1023, its 64-record blocks counted from record 1
        zeros = ((0 if place == "head_lane0" else 63) - t) % 64
        if start + zeros + t > ID_CH - 1:
            return None
    else:
        want = {"chunk_first": 0, "chunk_last": ID_CH - 1, "lane0": 5 * 64, "lane63": 5 * 64 + 63, "tail": 7}[place]
        start = 3 + k % 5                              # the contig starts inside chunk 0, the tie's chunk lies behind whole chunks of it
        g = max(start + t, ID_CH if place != "tail" else 2 * ID_CH)
        g += (want - g) % ID_CH                        # the sample index of the tie
        zeros = g - start - t
    front = [ZERO] * zeros + core
    S = replay(front)[0][-1]
    pair = tie_pair(e, k)
    S += identity(*pair)
    room = []
    while len(room) < AFTER:
        f = _no_tie_filler(S, len(room))
        if S + identity(*f) >= 2.0 ** (e + 1) - 1.0:
            break
        S += identity(*f)
        room.append(f)
    n_behind = AFTER + ID_CH if place.startswith("head") else AFTER      # behind a head at least one whole chunk, or there is no head
    behind = room[:100] if place == "tail" else room + [ZERO] * (n_behind - len(room))
    return front + [pair] + behind, start, len(front)


def _with_starts(cases):
    """Chains back to back in one sample, each behind a contig of as many filler records as it takes for its first record to be record
    `start` (mod 1024) of the sample.  Returns (sample, [first record index of each chain])."""
    parts, firsts, total = [], [], 0
    for values, start in cases:
        lead = (start - total) % ID_CH
        parts.append(identity_chain(values, lead))
        firsts.append(total + lead)
        total += lead + len(values)
    return concat(parts), firsts


def tie_sample(e):
    """Every tie case of binade e in one sample: (sample, [(place, values, first record index, index of the tie in values)])."""
    cases = [(p, tie_case(e, p, k)) for k, p in enumerate(TIE_PLACES)]
    cases = [(p, c) for p, c in cases if c is not None]
    b, firsts = _with_starts([(c[0], c[1]) for _, c in cases])
    return b, [(p, c[0], f, c[2]) for (p, c), f in zip(cases, firsts)]


def power_of_two_values():
    """4 096 records of identity 1.0, then 2 000 fillers: from record 0 the sum is exactly 2^11 after chunk 1 and 2^12 after chunk 3."""
    return [ONE] * 4096 + filler(2000)


def power_of_two_sample(start):
    """start = 0: the record that lifts the sum to 2^k is lane 63 of its 64-record block (k >= 6); start = 1: lane 0 (of the first block of
    chunks 1, 2 and 4: their sums cross a binade, so they are replayed serially)."""
    return _with_starts([(power_of_two_values(), start)])[0]


LAYOUT_COUNTS = (1025, 1023, 2047, 1, 2048, 63, 3073, 2049, 64, 1024, 65)


def layout_sample():
    """Contigs back to back with the read counts of LAYOUT_COUNTS, in that order: (sample, [(first record, records)])."""
    spans, total = [], 0
    for n in LAYOUT_COUNTS:
        spans.append((total, n))
        total += n
    return concat([identity_chain(filler(n, 3 * k)) for k, n in enumerate(LAYOUT_COUNTS)]), spans


def batches_sample(n_chunks):
    """One contig with n_chunks interior chunks (it starts at record 3 and ends 5 records into a chunk).  129 chunks: seven records of
    1.0 to every filler, so that the sum reaches binade 17."""
    n = (ID_CH - 3) + n_chunks * ID_CH + 5
    values = filler(n) if n_chunks < 129 else [ONE if i % 8 else filler(1, i)[0] for i in range(n)]
    return _with_starts([(values, 3)])[0], values


def uncounted_sample():
    """Supplementary, secondary and unmapped records inside interior chunks and on chunk borders, one record of identity 0.0 and one of
    negative identity (NM > aligned) in an interior chunk while the sum is above 4 096: (sample, values, flags)."""
    values = filler(7000)
    flags = {}
    for i, f in ((1021 + 300, 0x800), (1021 + 1023, 0x800), (1021 + 1024, 0x100), (1021 + 2047, 0x4), (1021 + 2048, 0x800), (1021 + 2500, 0x100),
                 (1021 + 2600, 0x4), (1021 + 3071, 0x100), (1021 + 3072, 0x4), (5, 0x800), (6999, 0x800)):
        flags[i] = f                                   # the contig starts at record 3: index 1021 + j is record j of chunk 1
    values[1021 + 700] = ZERO
    values[1021 + 4 * ID_CH + 500] = (FILLER_ALIGNED, 130)          # identity -0.3
    parts = [identity_chain(filler(3)), identity_chain(values, flags=flags)]
    return concat(parts), values, flags


# ------------------------------------------------------------------------------------------------ estimator cases
TRIM = (0.05, 0.95)
T0 = 4000
START_BINS = (0, 1, 62, 63, 64, 65, 95, 96, 97, 127, 128, 200)
TRIM_PAIRS = ((0.05, 0.95), (0.1, 0.9), (0.0, 1.0), (0.5, 0.5), (0.9, 0.1), (0.25, 0.75), (0.0, 0.01), (0.99, 1.0))      # test_gpu_estimates.estimator_sets
NO_END = (0.05, 0.99995)         # ceil(0.99995 * 4000 as f32) == 4000: the last prefix equals max_index


class Case:
    """One contig: its window histogram `counts`, the trim pair it is built for and what it claims about the walk:
    s, e (walk_points), ps = P[s] - min_index, pe = P[e-1] - max_index (where e lies behind s), plast = P[last] - max_index."""
    def __init__(self, name, counts, trim=TRIM, s=None, e=None, ps=None, pe=None, plast=None, **stair):
        self.name, self.counts, self.trim, self.s, self.e, self.ps, self.pe, self.plast, self.stair = name, as_counts(counts), trim, s, e, ps, pe, plast, stair
        self.T = sum(self.counts.values())

    def bam(self, excl):
        kw = dict(self.stair)
        if "cut_left" in kw:
            kw["cut_left"] = min(kw["cut_left"], excl)
        return staircase(self.counts, excl, **kw)


def _tc(name, T, trim, s, e, dv=0, ev=0, **kw):
    c = trimmed_counts(T, trim, s, e, dv, ev, **kw)
    between = e is not None and e > s + 1
    return Case(name, c, trim, s, e, ps=(dv if between or e is None else None), pe=(-ev if e is not None and e > s else None))


def start_cases():
    """The start bin s at every lane and batch that matters; P[s] == min_index and min_index + 1, P[s-1] == min_index - 1."""
    return [_tc("start_s%d_dv%d" % (s, dv), T0, TRIM, s, s + 2, dv, 0, last=s + 3) for s in START_BINS for dv in (0, 1)]


def end_cases():
    """The end bin e: the start bin itself, the next bin, lane 0 of the next batch, three batches on, none; P[e-1] == max_index and
    max_index - 1; runs of empty bins between s and e."""
    out = []
    for s in (1, 63, 70):
        nxt = 64 * (s // 64 + 1)
        out.append(_tc("end_s%d_same" % s, T0, TRIM, s, s, last=s + 70))
        for ev in (0, 1):
            out.append(_tc("end_s%d_next_ev%d" % (s, ev), T0, TRIM, s, s + 1, 0, ev, last=s + 2))
            if nxt > s + 1:
                out.append(_tc("end_s%d_lane0_ev%d" % (s, ev), T0, TRIM, s, nxt, 0, ev, last=nxt + 1))
            out.append(_tc("end_s%d_3batches_ev%d" % (s, ev), T0, TRIM, s, nxt + 128 + 5, 1, ev, last=nxt + 140, mids=(s + 2, nxt + 64)))
        c = _tc("end_s%d_none_last_is_max" % s, T0, NO_END, s, None, 0, last=s + 66, mids=(s + 1,))
        c.plast = 0
        out.append(c)
        out.append(_tc("end_s%d_trim_max_one" % s, T0, (0.05, 1.0), s, None, 1, last=s + 66, mids=(s + 1,)))
    return out


def bin_count_cases():
    """2, 64, 65, 96, 97, 128 and 129 bins, every one occupied; 300 bins and 600 bins (above the 512 of the LDS histogram), sparse."""
    out = []
    for nh in (2, 64, 65, 96, 97, 128, 129):
        s, e = (0, 1) if nh == 2 else (nh // 3, nh - 2)
        for ev in (0, 1):
            out.append(_tc("bins%d_ev%d" % (nh, ev), T0, TRIM, s, e, 0, ev, last=nh - 1, mids=range(nh)))
    out.append(_tc("bins300", T0, TRIM, 130, 260, 0, 0, last=299, mids=(5, 64, 128, 131, 192, 258)))
    out.append(_tc("bins600", T0, TRIM, 200, 520, 1, 1, last=599, mids=(64, 300, 511, 512, 513)))
    return out


def trim_pair_cases():
    """Indices that coincide (the mean divides by zero), trim_min = 0 over an empty bin 0, the other pairs of the goldens at their own
    indices.  (min > max, 0.9 / 0.1, has no walk to place: every case of every family is evaluated with it.)"""
    out = [_tc("pair_equal_indices_T%d" % T, T, (0.5, 0.5), 3, 4, 0, 0, last=6) for T in (T0, T0 + 1)]
    out.append(_tc("pair_min0_empty_bin0", T0, (0.0, 1.0), 0, None, 0, last=5, mids=(1, 2, 3)))
    out.append(_tc("pair_0_001", T0, (0.0, 0.01), 0, 2, 0, 0, last=4))
    out.append(_tc("pair_01_09", T0, (0.1, 0.9), 3, 6, 0, 0, last=8))
    out.append(_tc("pair_025_075", T0, (0.25, 0.75), 3, 66, 1, 1, last=70))
    out.append(_tc("pair_099_1", T0, (0.99, 1.0), 2, None, 0, last=3))
    return out


def bin0_extra_cases():
    """Three or more untouched 1024-base tiles in the middle and at the end; the window's border cutting through the first segment."""
    c = {0: 9000, 1: 500, 2: 400, 3: 300, 4: 200, 5: 100}
    return [Case("tiles_untouched", c, pad_left=100, mid=4200, mid_after=2),
            Case("border_cuts_segment", c, pad_left=0, mid=4300, mid_after=3, cut_left=30)]


def variance_cases():
    return [Case("covered_everywhere", {3: 500, 4: 700, 7: 300}), Case("one_uncovered_base", {0: 1, 3: 500, 4: 700, 7: 299}, mid=1, mid_after=3),
            Case("T1", {2: 1}), Case("T2", {1: 1, 2: 1}), Case("T3", {1: 1, 2: 1, 4: 1})]


def min_fraction_case():
    return Case("min_fraction", {0: 1234, 1: 2000, 2: 766}, pad_left=34, nm=1)


def long_contig_case():
    """A window of 2^24 + 3 bases, which f32 rounds to 2^24 + 4, with two small piles."""
    T = (1 << 24) + 3
    return Case("long", {0: T - 80, 1: 50, 2: 30}, pad_left=1000, mid=8_000_000, mid_after=1, nm=2)


FAMILIES = {"start": start_cases, "end": end_cases, "bins": bin_count_cases, "pairs": trim_pair_cases, "bin0_extra": bin0_extra_cases,
            "variance": variance_cases}


def family_sample(family, excl):
    """The cases of one family in one sample, a contig without reads or a contig shorter than 2 x 75 with reads between them:
    (sample, {tid: Case})."""
    parts, where = [bare(3000)], {}
    for k, c in enumerate(FAMILIES[family]()):
        where[len(parts)] = c
        parts.append(c.bam(excl))
        parts.append(short_with_reads() if k % 2 else bare(max(1, 2 * excl - 1 + k % 3)))
    parts.append(short_with_reads())
    return concat(parts), where



# ------------------------------------------------------------------------------------------------ genome cases
GENOME_TRIM = (0.5, 0.95)        # min_index lies above the unobserved bases, so that bin 0 can be placed on either side of it
GENOME_T = 12000


def unobserved_lengths(excl):
    """Contigs without reads of 1, 2 x excl - 1, 2 x excl, 2 x excl + 1 and 5 000 bases (at least 1)."""
    return [1, max(1, 2 * excl - 1), max(1, 2 * excl), 2 * excl + 1, 5000]


def unobserved_bases(lens, excl):
    """estimators.rs:226-242: a contig shorter than 2 x excl counts whole."""
    return sum(n if n < 2 * excl else n - 2 * excl for n in lens)


def genome_bin0_cases(excl):
    """One staircase contig per genome; with the genome's unobserved bases in bin 0 the MERGED histogram stands in the relation named
    (T = window + unobserved bases): [(Case of the merged histogram, Case of the contig)]."""
    U = unobserved_bases(unobserved_lengths(excl), excl)
    out = []
    for name, s, e, dv, ev in (("g_s0_dv0", 0, 3, 0, 0), ("g_s0_dv1", 0, 3, 1, 1), ("g_s1_dv0", 1, 4, 0, 0), ("g_s1_dv1", 1, 4, 1, 1),
                               ("g_s0_same", 0, 0, 0, 0), ("g_s0_next_ev0", 0, 1, 0, 0), ("g_s0_next_ev1", 0, 1, 0, 1), ("g_s1_s97", 1, 97, 0, 0)):
        merged = _tc(name, GENOME_T, GENOME_TRIM, s, e, dv, ev, last=max(s, e) + 2)
        own = dict(merged.counts)
        own[0] -= U
        assert own[0] >= 0
        out.append((merged, Case(name, own, GENOME_TRIM, pad_left=own[0] // 2)))
    return out


def genome_sample(excl):
    """(sample, genome_of_tid, n_genomes, {genome: (merged Case, tid of its staircase, its unobserved lengths)}).
    Genomes 0 .. 7: one staircase contig with the unobserved contigs in front of it and behind it.  Then a genome of two observed contigs
    with different bin counts, an observed contig shorter than 2 x 75 and an unobserved one; a genome of 300 contigs (two segments of 256)
    with observed contigs in both and unobserved ones between them; a genome without an observed contig; one without a contig; and a
    contig outside every genome."""
    parts, g_of, single = [], [], {}
    un = unobserved_lengths(excl)
    for g, (merged, own) in enumerate(genome_bin0_cases(excl)):
        single[g] = (merged, len(parts) + 2, un)
        parts += [bare(un[0]), bare(un[1]), own.bam(excl), bare(un[2]), bare(un[3]), bare(un[4])]
        g_of += [g] * 6
    g = len(single)
    parts += [staircase({0: 40, 1: 30, 69: 20}, excl, pad_left=7), bare(500), staircase({0: 3, 2: 50, 5: 10, 129: 9}, excl, nm=1), short_with_reads()]
    g_of += [g] * 4
    parts.append(staircase({0: 10, 1: 10}, excl))
    g_of.append(-1)
    g += 1
    observed = {0: {1: 30, 3: 5}, 5: {0: 9, 2: 40}, 100: {0: 50, 1: 30, 97: 20}, 255: {0: 1, 64: 12}, 256: {0: 5, 1: 5, 130: 7}, 299: {0: 20, 4: 4, 96: 3}}
    for k in range(300):
        parts.append(staircase(observed[k], excl) if k in observed else bare((149, 150, 151, 1000, 1)[k % 5]))
        g_of.append(g)
    g += 1
    parts += [bare(150), bare(3000)]
    g_of += [g, g]
    return concat(parts), np.asarray(g_of, np.int32), g + 2, single
