"""What a depth region is, in numpy, and what the depth-region tests share (CPU emulation, BED reader and formatter, device and CLI)."""
import numpy as np

from tests import depth_bins_ref as B

BIN_DTYPE = B.BIN_DTYPE
VALUES = B.VALUES
W = B.stretch_bases()      # dbnc::STRETCH_BASES: the bases of one piece of a region (a wave's 16 loads of 64 words)


def region_sets(lens, seed=1):
    """name -> list of (tid, start, end), deterministic, for targets of lengths `lens` ([start, end), 0-based, start < end <= length)."""
    lens = [int(L) for L in lens]
    live = [t for t, L in enumerate(lens) if L > 0]
    out = {}
    # edges: all four word residues at both ends, regions inside one word, the first and the last base, the whole target
    edges = []
    for t in live:
        L = lens[t]
        edges += [(t, 0, L), (t, 0, 1), (t, L - 1, L)]
        edges += [(t, a, e) for a in range(0, min(5, L - 1) + 1) for e in range(max(a + 1, L - 5), L + 1)]
    out["edges"] = edges
    # steps: a wave load's 256-base boundary from both sides
    out["steps"] = [(t, a, a + n) for t in live if lens[t] >= 600 for a in (0, 1, 2, 3, 253, 255, 256, 257) for n in (1, 3, 4, 5, 255, 256, 257, 511, 513)]
    # pieces: with skip = 3, len = W - 3 is exactly one piece and len = W - 2 adds a second piece that holds one base
    pieces = []
    for t in live:
        if lens[t] >= 3 * W:
            pieces += [(t, a, a + n) for a in (0, 1, 2, 3) for n in (W - 4, W - 3, W - 2, W - 1, W, W + 1, W + 3, W + 4, 2 * W, 2 * W + 7)]
            pieces.append((t, 0, lens[t]))
    out["pieces"] = pieces
    # overlap: one region three times, nested regions, targets interleaved, then the whole list once more reversed
    per = []
    for t in live:
        L = lens[t]
        nest = [(t, 0, L)]
        a, e = 0, L
        while e - a > 2:      # each strictly inside the one in front
            a, e = a + max(1, (e - a) // 5), e - max(1, (e - a) // 7)
            nest.append((t, a, e))
        per.append(nest)
    inter = [p[k] for k in range(max((len(p) for p in per), default=0)) for p in reversed(per) if k < len(p)]      # round robin, the last target first
    big = max(live, key=lambda t: lens[t]) if live else None
    over = inter + ([(big, 0, lens[big])] * 3 if live else [])
    out["overlap"] = over + over[::-1]
    # random
    rng = np.random.default_rng(seed)
    rnd = []
    for _ in range(300 if live else 0):
        t = live[int(rng.integers(0, len(live)))]
        a = int(rng.integers(0, lens[t]))
        e = int(rng.integers(a + 1, lens[t] + 1))
        rnd.append((t, a, e))
    out["random"] = rnd
    return out


def reduce(depths, regions):
    """The fields of every region, in the order given: slices of the per-target depth."""
    r = np.zeros(len(regions), BIN_DTYPE)
    for i, (t, a, e) in enumerate(regions):
        d = np.asarray(depths[t][a:e], np.int64)
        assert len(d) == e - a and e > a
        r["sum"][i], r["min"][i], r["max"][i], r["covered"][i] = d.sum(), d.min(), d.max(), (d > 0).sum()
    return r


def pieces_of(a, e):
    """Pieces of [a, e): its arena words counted from the word that holds `a`, cut every W / 4 words."""
    words = ((a % 4) + (e - a) + 3) // 4
    return (words + W // 4 - 1) // (W // 4)


def bed_lines(names, regions, region_names=None):
    """The BED text of `regions`; region_names[i] (None: no fourth field) is the name of line i."""
    out = []
    for i, (t, a, e) in enumerate(regions):
        nm = region_names[i] if region_names else None
        out.append("%s\t%d\t%d%s\n" % (names[t], a, e, "" if nm is None else "\t" + nm))
    return "".join(out)


def render(names, regions, res, value="mean", no_zeros=False, region_names=None):
    """The lines `coverm-amd depth --regions` writes for one sample (without the track line), in the file's order."""
    out = []
    for i, (t, a, e) in enumerate(regions):
        if no_zeros and res["max"][i] == 0:
            continue
        v = "%.3f" % (int(res["sum"][i]) / (e - a)) if value == "mean" else "%d" % int(res[value][i])
        nm = region_names[i] if region_names else None
        out.append("%s\t%d\t%d\t%s%s\n" % (names[t], a, e, "" if nm is None else nm + "\t", v))
    return "".join(out)
