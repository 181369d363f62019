"""Helpers of the --unsorted / cov_group_records tests: shuffled inputs made from sorted ones, and the expected side — the same records in
the stable grouped order, computed with numpy alone (never with the code under test)."""
import numpy as np

from coverm_amd.engine import RecordBatch
from oracle.bamio import BamData


def keys(tid, n_targets):
    """rec_key's order: a reference's tid, n_targets for a record without a reference."""
    t = np.asarray(tid, np.int64)
    return np.where((t >= 0) & (t < n_targets), t, n_targets)


def grouped_order(tid, n_targets):
    return np.argsort(keys(tid, n_targets), kind="stable")


def _cigar_take(cigar_off, cigar, perm):
    co = np.asarray(cigar_off, np.int64)
    n = co[1:] - co[:-1]
    new_off = np.zeros(len(perm) + 1, np.int64)
    np.cumsum(n[perm], out=new_off[1:])
    total = int(new_off[-1])
    src = np.repeat(co[:-1][perm] - new_off[:-1], n[perm]) + np.arange(total, dtype=np.int64)
    return new_off.astype(np.uint32), np.asarray(cigar, np.uint32)[src] if total else np.zeros(0, np.uint32)


def take_batch(b: RecordBatch, perm) -> RecordBatch:
    perm = np.asarray(perm, np.int64)
    off, cig = _cigar_take(b.cigar_off, b.cigar, perm)
    return RecordBatch.from_arrays(b.tid[perm], b.pos[perm], b.flag[perm], b.mapq[perm], b.nm[perm], b.nm_kind[perm], b.l_seq[perm], off, cig)


def take_bamdata(d: BamData, perm) -> BamData:
    perm = np.asarray(perm, np.int64)
    off, cig = _cigar_take(d.cigar_off, d.cigar, perm)
    f = lambda a: np.asarray(a)[perm]
    return BamData(list(d.ref_names), d.ref_lens, f(d.tid), f(d.pos), f(d.flag), f(d.mapq), f(d.l_seq), f(d.nm), f(d.nm_kind), off, cig, f(d.mtid), f(d.mpos),
                   f(d.tlen), [d.qname[i] for i in perm] if len(d.qname) else [], d.header_text)


def shuffles(n, seed, names=None):
    """The three shuffles of the issue: a random permutation; name order (mates adjacent: a mapper's output) — a stable sort by read name
    when names are known, else pairs of neighbours dealt at random; whole blocks of 1 000 records swapped."""
    rng = np.random.default_rng(seed)
    out = {"random": rng.permutation(n)}
    if names is not None and len(names) == n:
        out["name"] = np.asarray(sorted(range(n), key=lambda i: (names[i], i)), np.int64)
    else:
        pairs = rng.permutation((n + 1) // 2)
        out["name"] = np.stack([2 * pairs, 2 * pairs + 1], 1).reshape(-1)
        out["name"] = out["name"][out["name"] < n]
    blocks = [np.arange(lo, min(n, lo + 1000)) for lo in range(0, n, 1000)]
    out["blocks"] = np.concatenate([blocks[i] for i in rng.permutation(len(blocks))]) if blocks else np.zeros(0, np.int64)
    return out


def assert_same_records(got: RecordBatch, want: RecordBatch):
    for f in ("tid", "pos", "flag", "mapq", "nm", "nm_kind", "l_seq", "cigar_off", "cigar"):
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == b.dtype and a.shape == b.shape, f
        assert a.tobytes() == b.tobytes(), f
