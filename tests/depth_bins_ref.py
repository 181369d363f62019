"""What a depth bin is, in numpy, and what the depth-bin tests share (CPU emulation, formatter, device and CLI)."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BIN_DTYPE = np.dtype([("sum", "<u8"), ("min", "<i4"), ("max", "<i4"), ("covered", "<u4"), ("reserved", "<u4")])
VALUES = ("mean", "sum", "min", "max", "covered")


def stretch_bases():
    """dbnc::STRETCH_BASES, the width of a wave's stretch of the arena in bases, read from the header that names it."""
    text = open(os.path.join(ROOT, "coverm_amd", "csrc", "depth_bins_core.h")).read()
    steps = int(re.search(r"constexpr u32 WAVE_STEPS = (\d+);", text).group(1))
    assert re.search(r"constexpr u32 STRETCH_WORDS = 64u \* WAVE_STEPS;", text) and re.search(r"constexpr u32 STRETCH_BASES = 4u \* STRETCH_WORDS;", text)
    return 4 * 64 * steps


def bins_of(depths, B):
    """(bin_off, bins) over a list of per-target depth arrays: ceil(L / B) bins per target, never across a target boundary."""
    off, parts = [0], []
    for d in depths:
        d = np.asarray(d, np.int64)
        L = len(d)
        n = (L + B - 1) // B
        b = np.zeros(n, BIN_DTYPE)
        if n:
            cuts = np.arange(0, L, B)
            b["sum"] = np.add.reduceat(d, cuts)
            b["min"] = np.minimum.reduceat(d, cuts)
            b["max"] = np.maximum.reduceat(d, cuts)
            b["covered"] = np.add.reduceat((d > 0).astype(np.int64), cuts)
        parts.append(b)
        off.append(off[-1] + n)
    return np.asarray(off, np.uint64), (np.concatenate(parts) if parts else np.zeros(0, BIN_DTYPE))


def bin_lengths(lens, B):
    return [min((b + 1) * B, int(L)) - b * B for L in lens for b in range((int(L) + B - 1) // B)]


def bedgraph(names, lens, bin_off, bins, B, value="mean", no_zeros=False):
    """The lines `coverm-amd depth --bin-size B --bin-value value` writes for one sample (without the track line)."""
    out = []
    for t, name in enumerate(names):
        for j in range(int(bin_off[t]), int(bin_off[t + 1])):
            start = (j - int(bin_off[t])) * B
            end = min(start + B, int(lens[t]))
            if no_zeros and bins["max"][j] == 0:
                continue
            v = "%.3f" % (int(bins["sum"][j]) / (end - start)) if value == "mean" else "%d" % int(bins[value][j])
            out.append("%s\t%d\t%d\t%s\n" % (name, start, end, v))
    return "".join(out)
