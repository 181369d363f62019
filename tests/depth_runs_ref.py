"""What a depth run is, in numpy, and the shapes the depth-run tests share (CPU emulation and device)."""
import numpy as np


def rle(depth):
    """(start, depth) of the maximal stretches of equal depth of one target."""
    d = np.asarray(depth)
    if d.size == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.int32)
    start = np.concatenate([[0], np.flatnonzero(np.diff(d)) + 1])
    return start.astype(np.uint32), d[start].astype(np.int32)


def runs_of(depths):
    """(run_off, start, depth) over a list of per-target depth arrays: the runs never cross a target boundary."""
    parts = [rle(d) for d in depths]
    off = np.concatenate([[0], np.cumsum([len(s) for s, _ in parts])]).astype(np.uint64)
    cat = lambda k, dt: np.concatenate([p[k] for p in parts]).astype(dt) if parts else np.zeros(0, dt)
    return off, cat(0, np.uint32), cat(1, np.int32)


def bedgraph(names, lens, run_off, start, depth, no_zeros=False):
    """The lines `coverm-amd depth` writes for one sample (without the track line)."""
    out = []
    for t, name in enumerate(names):
        lo, hi = int(run_off[t]), int(run_off[t + 1])
        for j in range(lo, hi):
            end = int(start[j + 1]) if j + 1 < hi else int(lens[t])
            if no_zeros and depth[j] == 0:
                continue
            out.append("%s\t%d\t%d\t%d\n" % (name, start[j], end, depth[j]))
    return "".join(out)


# Boundaries of the run kernels' work split, in bases: a lane's word (4), a scan thread's 16 words (64), a wave of lane words (256), the
# pileup's tile (1024), a wave of the scan (4096) and its workgroup (16384).
BOUNDARIES = (4, 64, 256, 1024, 4096, 16384)
EDGE_LENGTHS = (0, 1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025)


def step_depth(length, change_points, rng=None):
    """A depth array that is constant between the given change points (values differ across every change)."""
    d = np.zeros(length, np.int32)
    v = 0
    prev = 0
    for c in sorted(set(int(c) for c in change_points if 0 < c < length)):
        d[prev:c] = v
        v = v + 1 if rng is None else v + int(rng.integers(1, 5))
        prev = c
    d[prev:] = v
    return d


def shapes(seed=1):
    """name -> list of per-target depth arrays."""
    rng = np.random.default_rng(seed)
    few = lambda L: np.repeat(rng.integers(0, 4, size=L // 3 + 1), 3)[:L].astype(np.int32)      # stretches of three, depth 0 .. 3
    out = {}
    out["edge_lengths"] = [few(L) for L in EDGE_LENGTHS]
    out["edge_lengths_reversed"] = [few(L) for L in reversed(EDGE_LENGTHS)]
    out["three_targets_in_a_word"] = [few(L) for L in (1, 1, 1, 1, 2, 1, 1, 1, 2, 3, 1, 1, 1)]
    out["starts_at_every_residue"] = [few(L) for L in (5, 6, 7, 8, 9, 1, 10, 2, 11, 3, 12, 4, 13)]
    out["equal_across_boundaries"] = [np.full(L, 3, np.int32) for L in (4, 8, 1, 5, 256, 1024, 3, 0, 7)]
    big = 3 * BOUNDARIES[-1] + 77
    crossing = [c for b in BOUNDARIES for c in (b - 2, b + 3, 2 * b, 3 * b - 1, 3 * b)]
    out["runs_cross_boundaries"] = [step_depth(big, crossing), step_depth(big, [b for b in BOUNDARIES]), step_depth(1025, [1023, 1024])]
    out["change_at_every_base"] = [(np.arange(L) % 5).astype(np.int32) for L in (1025, 5, 260)]
    out["all_zero"] = [np.zeros(L, np.int32) for L in (0, 1, 1024, 1025, 0, 3, 20000, 0)]
    out["empty_targets_only"] = [np.zeros(0, np.int32) for _ in range(5)]
    return out
