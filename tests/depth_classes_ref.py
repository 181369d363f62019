"""What a depth class, a run of depth classes and a threshold count are, in numpy, and what the depth-class tests share (CPU emulation,
formatters, device and CLI)."""
import numpy as np

from tests import depth_runs_ref as R

MAX_CUTS = 16
TOP_DEPTH = 2 ** 31 - 1

# The cut lists used throughout.
MIXED = (1, 2, 4, 16)                 # uncovered, 1, 2-3, 4-15, 16 and more: merges most depth changes of the shared shapes
ZERO_ONE = (0, 1)                     # class 1: uncovered, class 2: covered (class 0 stays empty)
UNIT = tuple(range(16))               # class = depth + 1 for depths <= 14: the class runs are the depth runs
TOP = (TOP_DEPTH,)                    # a single cut above every depth of the shapes
ONE = (3,)                            # a single cut
CUT_LISTS = {"MIXED": MIXED, "ZERO_ONE": ZERO_ONE, "UNIT": UNIT, "TOP": TOP, "ONE": ONE}


def class_of(d, cuts):
    """The number of cuts c with c <= d."""
    return np.searchsorted(np.asarray(cuts, np.int64), np.asarray(d, np.int64), side="right").astype(np.int32)


def class_runs_of(depths, cuts):
    """(run_off, start, cls) over a list of per-target depth arrays: the runs of equal class, never across a target boundary."""
    return R.runs_of([class_of(d, cuts) for d in depths])


def counts(depths, regions, thr):
    """uint32 (n_regions, K): per region and threshold, the bases of the slice with depth >= t."""
    out = np.zeros((len(regions), len(thr)), np.uint32)
    for i, (t, a, e) in enumerate(regions):
        d = np.asarray(depths[t][a:e], np.int64)
        for j, c in enumerate(thr):
            out[i, j] = (d >= c).sum()
    return out


def alternating_shape():
    """Every base changes depth, the class under MIXED changes exactly at b - 1, b and b + 1 for every b of R.BOUNDARIES (the depth alternates
    inside one class between two changes: 2, 3 in class 2, 4, 5 in class 3, 16, 17 in class 4), and the target behind starts in the class
    the first one ends in, which must not merge across the target boundary."""
    L = R.BOUNDARIES[-1] + 40
    pairs = {2: (2, 3), 3: (4, 5), 4: (16, 17)}
    changes = sorted({c for b in R.BOUNDARIES for c in (b - 1, b, b + 1)})
    d = np.zeros(L, np.int32)
    par = np.arange(L) & 1
    cls, prev = 2, 0
    for c in changes + [L]:
        lo, hi = pairs[cls]
        d[prev:c] = np.where(par[prev:c] == 0, lo, hi)
        prev, last = c, cls
        cls = 2 + (cls - 1) % 3
    lo, hi = pairs[last]
    first = hi if d[-1] == lo else lo      # same class as the base in front of it, another depth
    tail = np.where(np.arange(9) % 2 == 0, first, lo + hi - first).astype(np.int32)
    return [d, tail, np.zeros(0, np.int32), np.full(5, lo, np.int32)], changes


def shapes():
    """The shared shapes of tests/depth_runs_ref.py and the one of this module."""
    out = dict(R.shapes())
    out["alternating_in_class"] = alternating_shape()[0]
    return out


def _check_shapes():
    """The shapes are what the tests rely on (so they cannot drift away from it)."""
    d0, d1, _ = R.shapes()["runs_cross_boundaries"]
    s0, _ = R.rle(d0)
    c0, _ = R.rle(class_of(d0, MIXED))
    assert len(s0) == 31 and len(c0) == 5
    merged0 = set(s0.tolist()) - set(c0.tolist())
    assert len(merged0) == 26 and {8, 128, 512, 2048, 8192, 12288} <= merged0
    s1, _ = R.rle(d1)
    c1, _ = R.rle(class_of(d1, MIXED))
    assert set(s1.tolist()) - set(c1.tolist()) == {256, 4096, 16384}
    alt, changes = alternating_shape()
    a = alt[0]
    assert (np.diff(a) != 0).all()
    cs, cc = R.rle(class_of(a, MIXED))
    assert cs.tolist() == [0] + changes and (np.diff(cc) != 0).all()
    assert all(c in changes for b in R.BOUNDARIES for c in (b - 1, b, b + 1))
    assert class_of(a[-1:], MIXED)[0] == class_of(alt[1][:1], MIXED)[0] and a[-1] != alt[1][0]
    assert class_of(alt[1][-1:], MIXED)[0] == class_of(alt[3][:1], MIXED)[0]
    for name, dd in R.shapes().items():
        assert all(int(np.max(d, initial=0)) < TOP_DEPTH for d in dd), name


_check_shapes()


def parse_quantize(spec):
    """(cuts, open_end) of a --quantize spec; ValueError for a bad one."""
    f = spec.split(":")
    if len(f) < 2:
        raise ValueError("no class")
    open_end = f[-1] == ""
    if open_end:
        f = f[:-1]
    if f and f[0] == "":
        f[0] = "0"
    if not f or any(not x.isdigit() for x in f):
        raise ValueError("not a number")
    cuts = [int(x) for x in f]
    if len(cuts) > MAX_CUTS or any(c > TOP_DEPTH for c in cuts) or any(b <= a for a, b in zip(cuts, cuts[1:])):
        raise ValueError("bad cuts")
    if len(cuts) < 2 and not open_end:
        raise ValueError("no class")
    return tuple(cuts), open_end


def label(cuts, open_end, c):
    """The label of class c, or None when it is not printed."""
    n = len(cuts)
    if 1 <= c <= n - 1:
        return "%d:%d" % (cuts[c - 1], cuts[c])
    if c == n and open_end:
        return "%d:inf" % cuts[n - 1]
    return None


def render_classes(names, lens, run_off, start, cls, cuts, open_end):
    """The lines `coverm-amd depth --quantize` writes for one sample (without the track line)."""
    out = []
    for t, name in enumerate(names):
        lo, hi = int(run_off[t]), int(run_off[t + 1])
        for j in range(lo, hi):
            end = int(start[j + 1]) if j + 1 < hi else int(lens[t])
            lab = label(cuts, open_end, int(cls[j]))
            if lab is not None:
                out.append("%s\t%d\t%d\t%s\n" % (name, start[j], end, lab))
    return "".join(out)


def render_counts(names, regions, cnt, maxes=None, no_zeros=False, region_names=None):
    """The lines `coverm-amd depth --regions / --bin-size ... --thresholds` writes for one sample behind the track and #thresholds lines."""
    out = []
    for i, (t, a, e) in enumerate(regions):
        if no_zeros and maxes[i] == 0:
            continue
        nm = region_names[i] if region_names else None
        out.append("%s\t%d\t%d%s\t%s\n" % (names[t], a, e, "" if nm is None else "\t" + nm, "\t".join(str(int(c)) for c in cnt[i])))
    return "".join(out)
