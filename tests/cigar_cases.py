"""Inputs for the long-CIGAR path, each with a plain model of what its records must come to (no GPU, no kernel code).

The path decides what a record's CIGAR comes to and how its runs reach the pileup: cigar_sum3 / run_word (csrc/prep_lean.hip.h), the 32-bit
state machine of prep_step_generic and its copy in prep_body (k_prep7s), cigar_walk_wave / cigar_walk_slow, k_cx_expand with its bucket scan,
k_ranges, and apply / add_run of the three pileup kernels (csrc/pileup_kernels.hip.h).

`model_record` is the serial walk of oracle/coverm_oracle.c (cigar_walk: M = X add +1 at the cursor and -1 behind the operation, D and N move
the cursor, I S H P do not) told in runs, plus the "Run word" comment of pileup_kernels.hip.h: an M/=/X operation that starts where the
one before it ended continues its run (so runs with only I S H P between them merge, across zero-length operations as well), x = start of
the first run, SINGLE = one run, DOUBLE = two runs with len1 and len2 in 1..1023 and the gap in 1..255, everything else COMPLEX, or BUCKET
when the record has more than 16 operations and none of 2^24 bases.  A BUCKET record is expanded into one (tile, start, end) entry per
M/=/X operation of positive length and 1024-base tile it overlaps (clipped at the contig's length, the start inside the contig).

Every case puts its deviating records into a background of 100M reads, each at a chosen lane of a step of 64 records, and exists twice: as
a sample k_prep_lean takes (at least 128 records per contig) and with so many more (empty) contigs that it has fewer than 128 records per
contig, where k_prep_generic walks every step.  tests/test_cigar_cases.py checks on the CPU that each case has the property it is named
for; tests/test_gpu_cigar_paths.py runs them on the device.
"""
from bisect import bisect_right
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np

from coverm_amd.engine import RecordBatch
from oracle.bamio import BamData

TILE = 1024
CX_MIN_OPS = 16          # more operations than this: a record that is neither SINGLE nor DOUBLE goes through the buckets
CIG_FAST_OPS = 128       # more operations than this: the whole-wave walk
BIG = 1 << 24            # an operation of this many bases: the serial 64-bit walk, and never a bucket record
TYPE_BITS = {"SINGLE": 0, "DOUBLE": 1, "COMPLEX": 2, "BUCKET": 3}
LANES = (0, 31, 63)


def op(n, code):
    return (int(n) << 4) | "MIDNSHP=X".index(code)


def _batch(tid, pos, cigars, flag=None, nm=None, nm_kind=None, mapq=None, l_seq=None):
    n = len(tid)
    lens = np.fromiter((len(c) for c in cigars), dtype=np.int64, count=n)
    coff = np.zeros(n + 1, dtype=np.uint32)
    coff[1:] = np.cumsum(lens)
    cig = np.concatenate([np.asarray(c, dtype=np.uint32) for c in cigars]) if n else np.zeros(0, np.uint32)
    flag = np.zeros(n, np.uint16) if flag is None else np.asarray(flag, np.uint16)
    nm = np.ones(n, np.uint32) if nm is None else np.asarray(nm, np.uint32)
    nm_kind = np.ones(n, np.uint8) if nm_kind is None else np.asarray(nm_kind, np.uint8)
    mapq = np.full(n, 30, np.uint8) if mapq is None else np.asarray(mapq, np.uint8)
    l_seq = np.full(n, 100, np.int64) if l_seq is None else np.asarray(l_seq)
    return RecordBatch.from_arrays(np.asarray(tid, np.int32), np.asarray(pos, np.int32), flag, mapq, nm, nm_kind, l_seq, coff, cig)


def bamdata(batch: RecordBatch, ref_lens) -> BamData:
    n = batch.n_records
    z = np.zeros(n, np.int32)
    return BamData(["c%d" % i for i in range(len(ref_lens))], np.asarray(ref_lens, np.int64), batch.tid, batch.pos, batch.flag, batch.mapq,
                   batch.l_seq.astype(np.int32), batch.nm, batch.nm_kind, batch.cigar_off, batch.cigar, z, z, z, [b"r%d" % i for i in range(n)], "")


# ------------------------------------------------------------------------------------------------------------------ the model of one record
@dataclass
class Verdict:
    runs: List[Tuple[int, int]]          # merged M/=/X runs [start, end), not clipped
    aligned: int
    indel: int
    span: int
    n_ops: int
    big: bool
    kind: str                            # NONE, SINGLE, DOUBLE, COMPLEX, BUCKET
    word: int                            # x | y << 32
    entries: List[Tuple[int, int, int]]  # BUCKET records: (tile of the contig, start, end) k_cx_expand must write

    @property
    def n_runs(self):
        return len(self.runs)

    @property
    def len1(self):
        return self.runs[0][1] - self.runs[0][0]

    @property
    def len2(self):
        return self.runs[1][1] - self.runs[1][0]

    @property
    def gap(self):
        return self.runs[1][0] - self.runs[0][1]


def model_record(pos: int, ops, L: int) -> Verdict:
    """ops: [(length, code)].  Raises where the oracle reports an error (an M/=/X operation that starts outside the contig)."""
    cursor, cur_e = pos, None
    runs, per_op = [], []
    aligned = indel = 0
    big = False
    for ln, code in ops:
        big |= ln >= BIG
        if code in "M=X":
            if not 0 <= cursor < L:
                raise ValueError("M/=/X operation starts at %d, outside a contig of %d bases" % (cursor, L))
            if runs and cursor == cur_e:
                runs[-1][1] += ln
            else:
                runs.append([cursor, cursor + ln])
            cur_e = cursor + ln
            if ln > 0:
                per_op.append((cursor, cursor + ln))
            cursor += ln
            aligned += ln
        elif code == "D":
            cursor += ln; aligned += ln; indel += ln
        elif code == "N":
            cursor += ln
        elif code == "I":
            aligned += ln; indel += ln
        else:
            assert code in "SHP", code
    n_ops = len(ops)
    x, y, kind = 0, 0, "NONE"
    if runs:
        x = runs[0][0]
        l1 = runs[0][1] - runs[0][0]
        if len(runs) == 1:
            assert l1 < 1 << 30, "out of scope: a merged run of 2^30 bases"
            y, kind = l1, ("SINGLE" if l1 else "NONE")
        else:
            l2, gap = runs[1][1] - runs[1][0], runs[1][0] - runs[0][1]
            if len(runs) == 2 and 1 <= l1 <= 1023 and 1 <= l2 <= 1023 and 1 <= gap <= 255:
                kind, y = "DOUBLE", (1 << 30) | l1 | (gap << 10) | (l2 << 18)
            else:
                kind = "BUCKET" if n_ops > CX_MIN_OPS and not big else "COMPLEX"
                y = TYPE_BITS[kind] << 30
    entries = []
    if kind == "BUCKET":
        for s, e in per_op:
            for t in range(s // TILE, (min(e, L) - 1) // TILE + 1):
                entries.append((t, s, e))
    return Verdict([tuple(r) for r in runs], aligned, indel, cursor - pos, n_ops, big, kind, (x & 0xffffffff) | (y << 32), entries)


def decode_word(w: int):
    """A device run word as (kind, x, fields) for messages and field checks."""
    x, y = int(w) & 0xffffffff, int(w) >> 32
    if y == 0:
        return ("NONE", x, ())
    t = y >> 30
    if t == 0:
        return ("SINGLE", x, (y & 0x3fffffff,))
    if t == 1:
        return ("DOUBLE", x, (y & 1023, (y >> 10) & 255, (y >> 18) & 1023))
    return ("COMPLEX" if t == 2 else "BUCKET", x, (y & 0x3fffffff,))


# ------------------------------------------------------------------------------------------------------------------ a case
@dataclass
class Case:
    name: str
    ref_lens: np.ndarray
    recs: List[Tuple[int, int, list]]          # (tid, pos, [(length, code)]) in file order
    dev: List[int]                             # indices of the deviating records
    expect: List[dict]                         # per deviating record: what the case intends it to be (checked against the model on the CPU)
    verdicts: List[Verdict] = field(default_factory=list)
    small: bool = False
    depth_of: Tuple[int, ...] = (0, 1)
    case_property: Optional[Callable] = None   # a property of the whole sample, asserted on the model (CPU)
    slow_tiles: Optional[int] = None           # tiles k_pileup_fast must leave to k_pileup_stream, where the case is about that
    lanes_free: bool = False                   # the case places records by count, not by lane

    @property
    def n(self):
        return len(self.recs)

    def batch(self) -> RecordBatch:
        return _batch([r[0] for r in self.recs], [r[1] for r in self.recs], [[op(l, c) for l, c in r[2]] for r in self.recs])

    def bam(self) -> BamData:
        return bamdata(self.batch(), self.ref_lens)

    def tile_first(self):
        return np.concatenate([[0], np.cumsum((np.asarray(self.ref_lens, np.int64) + TILE - 1) // TILE)])

    def survives(self, v: Verdict, fp: Optional[dict]) -> bool:
        """The reader-stage single-read filter (length and percentage of the read; every record here has NM 1, l_seq 100, mapq 30)."""
        if not fp:
            return True
        a = v.aligned & 0xffffffff
        with np.errstate(divide="ignore", invalid="ignore"):
            return bool(a >= fp.get("min_aligned_length_single", 0)
                        and np.float32(a) / np.float32(100) >= np.float32(fp.get("min_aligned_percent_single", 0.0))
                        and np.float32(1.0) - np.float32(1) / np.float32(a) >= np.float32(fp.get("min_percent_identity_single", 0.0)))

    def words(self, fp: Optional[dict] = None) -> np.ndarray:
        return np.asarray([v.word if self.survives(v, fp) else 0 for v in self.verdicts], dtype=np.uint64)

    def bucket_records(self, fp=None) -> int:
        return sum(1 for v in self.verdicts if v.kind == "BUCKET" and self.survives(v, fp))

    def bucket_entries(self, fp=None) -> int:
        return sum(len(v.entries) for v in self.verdicts if self.survives(v, fp))

    def tile_entries(self) -> Dict[int, int]:
        """global tile -> bucket entries it receives"""
        tf, out = self.tile_first(), {}
        for (tid, _, _), v in zip(self.recs, self.verdicts):
            for t, _, _ in v.entries:
                out[int(tf[tid]) + t] = out.get(int(tf[tid]) + t, 0) + 1
        return out

    def tile_starts(self) -> Dict[int, int]:
        """global tile -> records that start in it (k_ranges' candidates of a tile no earlier record reaches into)"""
        tf, out = self.tile_first(), {}
        for tid, pos, _ in self.recs:
            k = int(tf[tid]) + min(pos, int(self.ref_lens[tid]) - 1) // TILE
            out[k] = out.get(k, 0) + 1
        return out

    def depth(self, tid: int) -> np.ndarray:
        L = int(self.ref_lens[tid])
        d = np.zeros(L + 1, np.int64)
        for (t, _, _), v in zip(self.recs, self.verdicts):
            if t == tid:
                for s, e in v.runs:
                    d[s] += 1
                    d[min(e, L)] -= 1
        return np.cumsum(d[:L]).astype(np.int32)


BG = [(100, "M")]


def background(L, n=1024, holes=()):
    """Start positions of n 100M reads at an even stride over [0, L - 100), none of them touching a hole [lo, hi)."""
    stride = max(1, (L - 100) // n)
    pos = [i * stride for i in range(n)]
    return [p for p in pos if not any(p < hi and p + 100 > lo for lo, hi in holes)]


def assemble(name, L0, devs, small, holes=(), n_bg=1024, bg=None, second=3000, more_contigs=(), dev_tid=0, **kw) -> Case:
    """devs: [(pos, ops, lane or None, expect)] on contig `dev_tid`.  Records are kept sorted by position; a deviating record reaches its
    lane through copies of the record in front of it (100M reads at that record's position)."""
    ref_lens = [L0, second] + list(more_contigs)
    per_contig: Dict[int, list] = {0: [(p, BG, None) for p in (background(L0, n_bg, holes) if bg is None else bg)],
                                   1: [(p, BG, None) for p in range(0, 64 * 40, 40)]}
    for c in range(2, len(ref_lens)):
        per_contig[c] = [(p, BG, None) for p in background(ref_lens[c], 256)]
    base = sum(len(per_contig[c]) for c in range(dev_tid))
    recs = per_contig[dev_tid]
    keys = [r[0] for r in recs]
    for j, (pos, ops, lane, _) in sorted(enumerate(devs), key=lambda d: d[1][0]):
        idx = bisect_right(keys, pos)
        if lane is not None:
            fill = (lane - (base + idx)) % 64
            fpos = keys[idx - 1] if idx else 0
            recs[idx:idx] = [(fpos, BG, None)] * fill
            keys[idx:idx] = [fpos] * fill
            idx += fill
        recs.insert(idx, (pos, ops, j))
        keys.insert(idx, pos)
    flat = [(c, p, o, j) for c in range(len(ref_lens)) for p, o, j in per_contig[c]]
    if small:      # fewer than 128 records per contig: contigs without a record behind the others
        ref_lens += [1500] * (len(flat) // 128 + 2 - len(ref_lens))
        assert len(flat) < 128 * len(ref_lens)
    else:
        assert len(flat) >= 128 * len(ref_lens)
    dev = [0] * len(devs)
    for i, r in enumerate(flat):
        if r[3] is not None:
            dev[r[3]] = i
    case = Case(name + ("-small" if small else ""), np.asarray(ref_lens, np.int64), [r[:3] for r in flat], dev, [d[3] for d in devs], small=small, **kw)
    case.verdicts = [model_record(p, o, int(case.ref_lens[c])) for c, p, o in case.recs]
    return case


# ------------------------------------------------------------------------------------------------------------------ CIGAR builders
JOIN = [(1, "I"), (2, "S"), (3, "H"), (1, "P")]


def pieces(total, k, codes="M=X"):
    """A run of `total` bases as k M/=/X operations (k <= max(total, 1)) joined by I, S, H and P: 2k - 1 operations."""
    k = max(1, min(k, total))
    base, extra = divmod(total, k)
    out = []
    for i in range(k):
        if i:
            out.append(JOIN[i % 4])
        out.append((base + (1 if i < extra else 0), codes[i % len(codes)]))
    return out


def pad_to(ops, n_ops):
    """More operations without another run: I S H P behind the last operation."""
    assert len(ops) <= n_ops, (len(ops), n_ops)
    return ops + [JOIN[i % 4] for i in range(n_ops - len(ops))]


def two_runs(len1, gap, gap_op, len2, n_ops):
    if n_ops == 3:
        return [(len1, "M"), (gap, gap_op), (len2, "=")]
    k = (n_ops - 1) // 4
    return pad_to(pieces(len1, k) + [(gap, gap_op)] + pieces(len2, k, "X=M"), n_ops)


def alternating(n_ops, m_len=7, special=None, codes="M"):
    """m_len M (or the codes in turn) at the even indices, 1I at the odd ones; special: {index: (length, code)}."""
    special = special or {}
    return [special[i] if i in special else ((m_len, codes[(i // 2) % len(codes)]) if i % 2 == 0 else (1, "I")) for i in range(n_ops)]


def spaced(devs, first=1500, step=3000):
    """(ops, expect) -> (pos, ops, lane, expect): one deviating record every `step` bases, the lanes 0, 31, 63 in turn."""
    return [(first + j * step, ops, LANES[j % 3], exp) for j, (ops, exp) in enumerate(devs)]


def expect_of(len1, gap, len2, n_ops):
    if 1 <= len1 <= 1023 and 1 <= gap <= 255 and 1 <= len2 <= 1023:
        return dict(kind="DOUBLE", len1=len1, gap=gap, len2=len2)
    return dict(kind="BUCKET" if n_ops > 16 else "COMPLEX", n_runs=2, len1=len1, gap=gap, len2=len2)


# ------------------------------------------------------------------------------------------------------------------ A: run-word classification
def case_fields(n_ops, small):
    """len1, gap (as D and as N) and len2 below, at and above what RW_DOUBLE's fields hold, one field at its edge at a time."""
    devs = []
    for len1 in (1, 1023, 1024):
        devs.append((two_runs(len1, 7, "D", 300, n_ops), expect_of(len1, 7, 300, n_ops)))
    for gap_op in "DN":
        for gap in (1, 255, 256):
            devs.append((two_runs(300, gap, gap_op, 200, n_ops), expect_of(300, gap, 200, n_ops)))
    for len2 in (1, 1023, 1024):
        devs.append((two_runs(300, 9, "N", len2, n_ops), expect_of(300, 9, len2, n_ops)))
    for ops, _ in devs:
        assert len(ops) == n_ops
    return assemble("fields-%dops" % n_ops, 40_000, spaced(devs), small)


def case_zero_length_and_no_match(small):
    devs = [
        ([(40, "M"), (0, "D"), (30, "M")], dict(kind="SINGLE", n_runs=1, len1=70)),
        ([(40, "M"), (0, "N"), (30, "M")], dict(kind="SINGLE", n_runs=1, len1=70)),
        ([(0, "M"), (5, "D"), (10, "M")], dict(kind="COMPLEX", n_runs=2, len1=0, len2=10)),
        ([(10, "M"), (0, "M"), (5, "D"), (0, "M"), (7, "=")], dict(kind="DOUBLE", len1=10, gap=5, len2=7)),
        ([(50, "S")], dict(kind="NONE", n_runs=0, aligned=0)),
        ([(20, "I"), (30, "S")], dict(kind="NONE", n_runs=0, aligned=20)),
        (pad_to([(20, "I"), (30, "S")], 20), dict(kind="NONE", n_runs=0)),
        (pad_to([(20, "I"), (30, "S")], 140), dict(kind="NONE", n_runs=0)),
        ([(0, "M")], dict(kind="NONE", n_runs=1, len1=0)),
        (pad_to([(0, "M"), (5, "D"), (10, "M")], 17), dict(kind="BUCKET", n_runs=2, len1=0)),
        (pad_to([(10, "M"), (0, "M"), (5, "D"), (0, "M"), (7, "=")], 130), dict(kind="DOUBLE", len1=10, gap=5, len2=7)),
    ]
    return assemble("zero-length-and-no-match", 40_000, spaced(devs), small)


# ------------------------------------------------------------------------------------------------------------------ B: operation counts
OP_COUNTS = (3, 4, 16, 17, 64, 65, 128, 129, 192, 193, 256, 257)


def case_op_counts(n_runs, small):
    """One record of each operation count among one-operation records: 5-base M/=/X operations joined by 1I, the runs split by 3D."""
    devs = []
    for n_ops in OP_COUNTS:
        n_m = (n_ops + 1) // 2
        if n_runs > n_m:
            continue          # (three operations hold two runs at most, and so do four)
        cut = {2 * (n_m * k // n_runs) - 1: (3, "D") for k in range(1, n_runs)}
        ops = alternating(n_ops, 5, cut, "M=X")
        lens = [5 * (n_m * (k + 1) // n_runs - n_m * k // n_runs) for k in range(n_runs)]
        if n_runs == 1:
            exp = dict(kind="SINGLE", n_runs=1, len1=lens[0], n_ops=n_ops)
        elif n_runs == 2:
            exp = dict(expect_of(lens[0], 3, lens[1], n_ops), n_ops=n_ops)
        else:
            exp = dict(kind="BUCKET" if n_ops > 16 else "COMPLEX", n_runs=3, len1=lens[0], len2=lens[1], n_ops=n_ops)
        devs.append((ops, exp))
    return assemble("op-counts-%druns" % n_runs, 40_000, spaced(devs), small)


# ------------------------------------------------------------------------------------------------------------------ C: the wave walk's bookkeeping
def case_gap_positions(n_gaps, m_len, small):
    """Records of 133 and 261 operations (m_len M, 1I in turn) whose only D is at a chosen operation index (an even index: the D stands in
    for the M there, between two I); with n_gaps == 2 a second gap 41 or 42 operations behind it (in front of it, where the record ends
    sooner) makes three runs.  m_len 7 keeps two runs inside RW_DOUBLE's fields, with m_len 40 one of them is always too long for them."""
    devs = []
    for n_ops, at in [(133, 1), (133, 62), (133, 63), (133, 64), (133, 65), (133, 127), (133, 128), (133, 129), (133, 131),
                      (261, 191), (261, 192), (261, 193), (261, 259)]:
        special = {at: (4, "D")}
        if n_gaps == 2:
            far = (at + 40) | 1
            special[far if far <= n_ops - 2 else 3] = (6, "D")
        ops = alternating(n_ops, m_len, special, "M=X")
        kind = "DOUBLE" if n_gaps == 1 and m_len * ((n_ops + 1) // 2) <= 1023 else "BUCKET"
        devs.append((ops, dict(gap_index=at, n_ops=n_ops, n_runs=n_gaps + 1, kind=kind)))
    return assemble("gap-at-index-%dgaps-%dM" % (n_gaps, m_len), 56_000, spaced(devs, 1000, 3900), small)


def case_first_match_and_run_starts(small):
    """The first M/=/X operation behind I operations only (index 0, 63, 64, 65, 130), the second run's first operation at lane 0 and at lane
    63 of a step of the walk, runs continued by = and X."""
    devs = []
    for lead in (0, 63, 64, 65, 130):
        ops = [(1, "I")] * lead + alternating(135 - min(lead, 5), 7, {61: (9, "D")}, "M=X")
        devs.append((ops, dict(first_match=lead, kind="DOUBLE", gap=9)))
        ops = [(1, "I")] * lead + alternating(135 - min(lead, 5), 20, {61: (9, "D"), 101: (300, "N")}, "M")
        devs.append((ops, dict(first_match=lead, kind="BUCKET", n_runs=3)))
    # run 2 begins at lane 0 of the second step: D at 63 (the operation in front of it), and D at 62 with an I between
    devs.append((alternating(140, 6, {63: (5, "D")}, "=XM"), dict(second_run_first_op=64, kind="DOUBLE", len1=32 * 6, gap=5, len2=38 * 6)))
    devs.append((alternating(140, 6, {62: (5, "D")}, "=XM"), dict(second_run_first_op=64, kind="DOUBLE", len1=31 * 6, gap=5, len2=38 * 6)))
    # ... and at lane 63 of the first step and of the second
    devs.append((alternating(140, 6, {62: (5, "D"), 63: (6, "X")}, "M"), dict(second_run_first_op=63, kind="DOUBLE", len1=31 * 6, gap=5, len2=39 * 6)))
    devs.append((alternating(140, 6, {126: (5, "D"), 127: (6, "X")}, "M"), dict(second_run_first_op=127, kind="DOUBLE", len1=63 * 6, gap=5, len2=7 * 6)))
    devs.append((alternating(257, 3, {126: (5, "N"), 127: (3, "=")}, "X"), dict(second_run_first_op=127, kind="DOUBLE", len1=63 * 3, gap=5, len2=66 * 3)))
    return assemble("first-match-and-run-starts", 60_000, spaced(devs, 1000, 3900), small)


# ------------------------------------------------------------------------------------------------------------------ D: several long records in a step
def long_record(k, n_ops=131):
    """A record of more than 128 operations; where its D sits, and so its runs, depends on k."""
    return alternating(n_ops, 7, {2 * (k % 60) + 1: (1 + k % 9, "D")}, "M=X")


def case_long_records_in_one_step(which, small, L0=40_000, neighbours=()):
    if which == "two":
        devs = [(20_000, long_record(3), 0, dict(kind="DOUBLE")), (20_000 + 63, long_record(40), 63, dict(kind="DOUBLE"))]
    elif which == "three":
        devs = [(20_000, long_record(17 + 20 * k, 131 + 64 * k), 30 + k, dict(kind="DOUBLE")) for k in range(3)]
    else:
        devs = [(20_000, long_record(k, 129 + k % 3), k, dict(kind="DOUBLE")) for k in range(64)]
    for k, (skip, n_ops) in enumerate(neighbours):      # between the two: a skip of 2^24 bases or one fewer, in 5 operations or in 130
        head = [(30, "M"), (skip, "N"), (40, "="), (5, "D"), (20, "X")]
        ops = head if n_ops == 5 else head + [(1, "I") if i % 2 == 0 else (2, "M") for i in range(n_ops - 5)]
        kind = "COMPLEX" if skip >= BIG or n_ops <= 16 else "BUCKET"
        devs.append((20_010 + k, ops, None, dict(kind=kind, n_runs=3, big=skip >= BIG, n_ops=n_ops)))
    return assemble("long-records-%s%s" % (which, "-skips-%dops" % neighbours[0][1] if neighbours else ""), L0, devs, small,
                    bg=background(40_000) if L0 > 40_000 else None)


# ------------------------------------------------------------------------------------------------------------------ E: k_cx_expand
BUCKET_HEAD = [(1, "M"), (1, "I")] * 8          # 16 operations, one run of 8 bases: with a skip and an M behind them a BUCKET record of 18


def bucket_record(start, m_start, m_len):
    """(pos, ops): 8 bases at `start`, then one M operation of m_len bases that starts at m_start (more than 255 bases further on)."""
    assert m_start - (start + 8) > 255
    return start, BUCKET_HEAD + [(m_start - start - 8, "N"), (m_len, "M")]


def case_one_operation_and_the_tile_borders(small):
    """One M operation of a BUCKET record against the 1024-base tiles: starts on a border, ends on one, one base past it, spans 1, 2 and 5."""
    L0 = 40_000
    devs = []
    for k, (m_start, m_len, tiles) in enumerate([(5 * TILE, 100, 1), (5 * TILE + 200, TILE - 200, 1), (5 * TILE + 200, TILE - 199, 2),
                                                 (7 * TILE, TILE, 1), (7 * TILE, TILE + 1, 2), (9 * TILE + 1000, 24 + 3 * TILE + 1, 5),
                                                 (9 * TILE - 1, 2, 2), (20 * TILE - 1, 1, 1)]):
        pos, ops = bucket_record(1000 + 450 * k, m_start, m_len)
        devs.append((pos, ops, LANES[k % 3], dict(kind="BUCKET", op_tiles=tiles, n_runs=2)))
    return assemble("one-operation-and-the-tile-borders", L0, devs, small)


def case_one_operation_and_the_contig_end(small):
    """ev == L, ev == L + 1, ev far beyond L; L is not a multiple of the tile, then it is."""
    devs = []
    L0 = 30 * TILE + 300
    for k, (m_start, m_len, tiles) in enumerate([(L0 - 50, 50, 1), (L0 - 50, 51, 1), (L0 - 700, 50_000, 2), (L0 - 1, 1, 1), (L0 - 1, 1 << 20, 1)]):
        pos, ops = bucket_record(2000 + 450 * k, m_start, m_len)
        devs.append((pos, ops, LANES[k % 3], dict(kind="BUCKET", op_tiles=tiles)))
    return assemble("one-operation-and-the-contig-end", L0, devs, small)


def case_one_operation_and_a_contig_end_on_a_border(small):
    devs = []
    L0 = 30 * TILE
    for k, (m_start, m_len, tiles) in enumerate([(L0 - 50, 50, 1), (L0 - 50, 51, 1), (L0 - TILE - 1, 3 * TILE, 2), (L0 - TILE, TILE, 1), (L0 - 1, 2, 1)]):
        pos, ops = bucket_record(2000 + 450 * k, m_start, m_len)
        devs.append((pos, ops, LANES[k % 3], dict(kind="BUCKET", op_tiles=tiles)))
    return assemble("one-operation-and-a-contig-end-on-a-border", L0, devs, small)


def many_operations(n_m, m_len=3, gaps=(9, 21)):
    """n_m M operations of m_len bases joined by 1I, two of the joints 2D instead: three runs, so a BUCKET record from 9 operations on."""
    return alternating(2 * n_m - 1, m_len, {2 * g + 1: (2, "D") for g in gaps}, "M=X")


def case_operations_in_tiles(which, small):
    """64 operations inside one tile; 64 over two tiles (a CIGAR only walks forward, so its operations cannot alternate between tiles:
    lanes 0-31 hit one tile, lane 32 straddles the border and hits both, lanes 33-63 the other — two keys in one ballot); 65 operations
    (one in the walk's second step); 2 and 8 such records over the same tiles, whose cursor atomics come from different waves."""
    T = 6 * TILE
    if which == "one-tile":
        devs = [(T + 100, many_operations(64), 31, dict(kind="BUCKET", n_runs=3))]
        prop = lambda c: _assert(c.tile_entries() == {6: 64})
    elif which == "two-tiles":
        # 32 operations of 3 bases and two D of 2 in front of lane 32's operation: it starts at T + TILE - 2 and ends at T + TILE + 1
        devs = [(T + TILE - 32 * 3 - 6, many_operations(64), 0, dict(kind="BUCKET", n_runs=3))]
        prop = lambda c: _assert(c.tile_entries() == {6: 33, 7: 32})
    elif which == "65":
        devs = [(T + 100, many_operations(65), 63, dict(kind="BUCKET", n_runs=3, n_ops=129))]
        prop = lambda c: _assert(c.tile_entries() == {6: 65})
    else:
        n = int(which)
        devs = [(T + TILE - 32 * 3 - 6 - 3 * k, many_operations(64 + k), None, dict(kind="BUCKET", n_runs=3)) for k in range(n)]
        prop = lambda c: _assert(sum(c.tile_entries().values()) == sum(64 + k for k in range(n)) + n and set(c.tile_entries()) == {6, 7})
    return assemble("operations-%s" % which, 40_000, devs, small, case_property=prop, lanes_free=which in ("2", "8"))


def case_bucket_offsets_past_a_scan_block(first_tiles, small):
    """The bucket offsets are a two-level scan (1024 tiles per block, cx.ctop[key >> 10] on top): a first contig of 1022 (2046) tiles, and in
    the second one a record whose operations fall into the global tiles 1022-1026 (2046-2050).  Depth of the second contig only."""
    L0, L1 = first_tiles * TILE, 6 * TILE + 77
    ops = []
    for t in range(5):          # in every tile: three operations joined by I, then a skip to the same offset of the next tile
        ops += [(30, "M"), (1, "I"), (40, "="), (2, "I"), (50, "X"), (TILE - 120, "N")]
    ops = ops[:-1]
    devs = [(100, ops, 31, dict(kind="BUCKET", n_runs=5)), (160, ops[:-6] + [(2000, "M")], 63, dict(kind="BUCKET", n_runs=4))]
    want = {first_tiles + t: (6 if t < 3 else 7 if t == 3 else 4) for t in range(5)}
    want[first_tiles + 5] = 1
    return assemble("bucket-offsets-past-%d-tiles" % first_tiles, L0, devs, small, second=L1, dev_tid=1, bg=[i * (L0 // 1100) for i in range(1024)],
                    depth_of=(1,), case_property=lambda c: _assert(c.tile_entries() == want, (c.tile_entries(), want)))


def _assert(ok, what=None):
    assert ok, what


# ------------------------------------------------------------------------------------------------------------------ F: consumption in the pileup
def case_double_and_complex_against_the_tiles(small):
    L0 = 40 * TILE - 300
    hi = 11 * TILE
    devs = []
    for d in (-1, 0, 1):         # the first run ends at the tile's hi - 1, hi, hi + 1
        devs.append((hi - 200 + d, [(200, "M"), (30, "D"), (150, "M")], dict(kind="DOUBLE", run1_end=hi + d)))
    devs.append((14 * TILE - 90, [(80, "M"), (20, "N"), (60, "M")], dict(kind="DOUBLE", gap_over=14 * TILE)))
    devs.append((17 * TILE - 150, [(100, "M"), (50, "D"), (70, "M")], dict(kind="DOUBLE", run2_start=17 * TILE)))
    devs.append((17 * TILE - 151, [(100, "M"), (50, "D"), (70, "M")], dict(kind="DOUBLE", run2_start=17 * TILE - 1)))
    devs.append((L0 - 400, [(300, "M"), (60, "N"), (500, "M")], dict(kind="DOUBLE", run2_past=L0)))
    devs.append((L0 - 130, [(100, "M"), (29, "N"), (1, "M")], dict(kind="DOUBLE", run2_end=L0)))
    devs.append((20 * TILE + 500, [(50, "M"), (1000, "N"), (50, "="), (1000, "N"), (50, "X")], dict(kind="COMPLEX", n_runs=3, tiles_of_runs=3)))
    devs.append((24 * TILE + 500, pad_to([(50, "M"), (1000, "N"), (50, "="), (1000, "N"), (50, "X"), (BIG, "S")], 19), dict(kind="COMPLEX", n_runs=3, big=True)))
    devs.append((28 * TILE + 500, pad_to([(50, "M"), (1000, "N"), (50, "="), (BIG + 5, "H"), (1000, "N"), (50, "X")], 140), dict(kind="COMPLEX", n_runs=3, big=True)))
    devs = [(p, o, LANES[k % 3], e) for k, (p, o, e) in enumerate(devs)]
    return assemble("double-and-complex-against-the-tiles", L0, devs, small)


def pile_record(start, at):
    """17 operations: 8 bases at `start` (eight 1M joined by 1I), a skip, 100M at `at`."""
    return start, [(1, "M"), (1, "I")] * 7 + [(1, "M"), (at - start - 8, "N"), (100, "M")]


def case_pile_of_bucket_entries(depth, where, small):
    """`depth` 17-operation records stacked on one spot of a tile no other record starts in or reaches: its candidates are bucket entries
    alone, `depth` of them, against k_pileup_fast's 512 LDS bins — in an interior tile and in the contig's last one."""
    L0 = 30 * TILE + 300
    t = 12 if where == "interior" else 30
    at = t * TILE + 150
    hole = [((t - 1) * TILE, (t + 1) * TILE)]
    devs = [pile_record(4 * TILE + 100, at) + (0 if k == 0 else None, dict(kind="BUCKET", n_runs=2)) for k in range(depth)]

    def prop(c):
        te, ts = c.tile_entries(), c.tile_starts()
        assert te == {4: 8 * depth, t: depth} and t not in ts and t - 1 not in ts, (te, ts.get(t))
        d = c.depth(0)
        assert d[at] == depth and d[at - 1] == 0 and d[at + 100] == 0 and d[(t - 1) * TILE:at].max() == 0
    return assemble("pile-of-%d-bucket-entries-%s" % (depth, where), L0, devs, small, holes=hole, case_property=prop, lanes_free=True)


def case_candidate_limit_with_bucket_entries(entries, small):
    """A tile of 8000 short reads and `entries` bucket entries: 8191 candidates stay with k_pileup_fast, 8192 go to k_pileup_stream."""
    L0 = 30 * TILE
    t = 12
    hole = [(t * TILE - 100, (t + 1) * TILE)]
    short = [(t * TILE + (k * 900) // 8000, [(60, "M")], None, dict(kind="SINGLE")) for k in range(8000)]
    devs = short + [pile_record(4 * TILE + 100, t * TILE + 300 + k) + (None, dict(kind="BUCKET")) for k in range(entries)]

    def prop(c):
        te, ts = c.tile_entries(), c.tile_starts()
        assert te[t] == entries and ts[t] == 8000 and ts.get(t - 1, 0) > 0
        assert not any(r[0] == 0 and r[1] < t * TILE and r[1] + v.span > t * TILE and v.kind != "BUCKET" for r, v in zip(c.recs, c.verdicts))
    return assemble("candidate-limit-8000-and-%d-entries" % entries, L0, devs, small, holes=hole, case_property=prop,
                    slow_tiles=1 if 8000 + entries > 8191 else 0, lanes_free=True)


# ------------------------------------------------------------------------------------------------------------------ G: the repeated pass
def case_bucket_entries_exactly(total, small=False):
    """BUCKET records of 64 entries each (and one of 64 + total % 64) that come to `total` entries."""
    n, rest = divmod(total, 64)
    assert n >= 2 and rest < 60
    # (the first record alone in a tile, four per tile behind it, none across a border: an operation in two tiles would be two entries)
    devs = [(3 * TILE + 100 if k == 0 else (4 + (k - 1) // 4) * TILE + 100 + 220 * ((k - 1) % 4), many_operations(64 + (rest if k == 0 else 0)), None,
             dict(kind="BUCKET")) for k in range(n)]
    return assemble("bucket-entries-%d" % total, 40_000, devs, small, case_property=lambda c: _assert(c.bucket_entries() == total), lanes_free=True)


# ------------------------------------------------------------------------------------------------------------------ H: the reader filter on the walked `aligned`
FILTER_ALIGNED = 62


def case_filter_on_each_walk(small):
    """One record through each of the four walks, every one with 62 aligned bases (l_seq 100): the closed form of three operations, the
    state machine, the whole-wave walk, and (an operation of 2^24 bases) the serial walk."""
    wave = [((1 if i < 120 else 0), "M") if i % 2 == 0 else ((1 if i in (1, 3) else 0), "I") for i in range(129)]
    devs = [([(30, "M"), (2, "D"), (30, "M")], dict(kind="DOUBLE", aligned=62, n_ops=3)),
            ([(10, "M"), (2, "I"), (20, "M"), (2, "D"), (28, "M")], dict(kind="DOUBLE", aligned=62, n_ops=5)),
            (wave, dict(kind="SINGLE", aligned=62, n_ops=129)),
            ([(30, "M"), (2, "D"), (30, "M"), (BIG, "S")], dict(kind="DOUBLE", aligned=62, big=True))]
    return assemble("filter-on-each-walk", 40_000, spaced(devs, 3000, 9000), small)


# ------------------------------------------------------------------------------------------------------------------ the list
BUILDERS: Dict[str, Callable[[bool], Case]] = {}
for _n in (3, 11, 40, 131):
    BUILDERS["fields-%dops" % _n] = (lambda small, n=_n: case_fields(n, small))
BUILDERS["zero-length-and-no-match"] = case_zero_length_and_no_match
for _r in (1, 2, 3):
    BUILDERS["op-counts-%druns" % _r] = (lambda small, r=_r: case_op_counts(r, small))
for _g in (1, 2):
    for _m in (7, 40):
        BUILDERS["gap-at-index-%dgaps-%dM" % (_g, _m)] = (lambda small, g=_g, m=_m: case_gap_positions(g, m, small))
BUILDERS["first-match-and-run-starts"] = case_first_match_and_run_starts
for _w in ("two", "three", "all-64"):
    BUILDERS["long-records-%s" % _w] = (lambda small, w=_w: case_long_records_in_one_step(w, small))
BUILDERS["one-operation-and-the-tile-borders"] = case_one_operation_and_the_tile_borders
BUILDERS["one-operation-and-the-contig-end"] = case_one_operation_and_the_contig_end
BUILDERS["one-operation-and-a-contig-end-on-a-border"] = case_one_operation_and_a_contig_end_on_a_border
for _w in ("one-tile", "two-tiles", "65", "2", "8"):
    BUILDERS["operations-%s" % _w] = (lambda small, w=_w: case_operations_in_tiles(w, small))
for _t in (1022, 2046):
    BUILDERS["bucket-offsets-past-%d-tiles" % _t] = (lambda small, t=_t: case_bucket_offsets_past_a_scan_block(t, small))
BUILDERS["double-and-complex-against-the-tiles"] = case_double_and_complex_against_the_tiles
for _d in (511, 512, 513):
    for _w in ("interior", "last-tile"):
        BUILDERS["pile-of-%d-bucket-entries-%s" % (_d, _w)] = (lambda small, d=_d, w=_w: case_pile_of_bucket_entries(d, w, small))
for _e in (191, 192):
    BUILDERS["candidate-limit-8000-and-%d-entries" % _e] = (lambda small, e=_e: case_candidate_limit_with_bucket_entries(e, small))
BUILDERS["filter-on-each-walk"] = case_filter_on_each_walk

# the two cases on a contig of 16.8 M bases (a skip of exactly 2^24 bases and one of 2^24 - 1 between two long records of one step)
HUGE_L = BIG + 100_000
HUGE_BUILDERS = {"long-records-two-skips-%dops" % n: (lambda small, n=n: case_long_records_in_one_step("two", small, L0=HUGE_L, neighbours=((BIG, n), (BIG - 1, n))))
                 for n in (5, 130)}

_cache: Dict[Tuple[str, bool], Case] = {}


def build(name: str, small: bool) -> Case:
    """Cases are built once and shared; nobody changes them."""
    key = (name, small)
    if key not in _cache:
        _cache[key] = (BUILDERS.get(name) or HUGE_BUILDERS[name])(small)
    return _cache[key]
