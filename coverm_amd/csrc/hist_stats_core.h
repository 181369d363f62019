// Window statistics of one contig read off its depth histogram.  With the histogram wanted, every window position of a tile the pileup
// visits lands in exactly one bin H[b] (b = its depth), so the bins determine what the pileup kernels would otherwise have to sum per
// position (pileup_kernels.hip.h):
//     sum_d    = sum over b of b * H[b]
//     sum_d2   = sum over b of b * b * H[b]      modulo 2^64, as `sum_d2 += (u64)d * d` per position wraps
//     cov_win  = sum over b > 0 of H[b]          covered window positions
//     proc_win = sum over b of H[b]              window positions of visited tiles (the rest of the window is at depth 0)
//     min_d / max_d = lowest / highest non-empty bin; 0xffffffff / 0 when no bin is set
// The rule is written once and run three ways: by one lane over all bins (k_estimate_lanes, k_hist_stats' shallow contigs), by the 64 lanes
// of a wave over bins lane, lane + 64, ... with `merge` across the lanes (k_estimate, k_hist_stats), and on the CPU by
// tests/c/hist_stats_host.cpp, which checks both forms against a loop over positions.
#pragma once
#include <stdint.h>

#ifndef HSTC_FN
#define HSTC_FN inline
#endif

namespace hstc {

typedef unsigned int u32;
typedef unsigned long long u64;

struct Stats {
    u64 sum_d, sum_d2, cov_win, proc_win;
    u32 min_d, max_d;
};

HSTC_FN Stats empty() { return Stats{0ull, 0ull, 0ull, 0ull, 0xffffffffu, 0u}; }

HSTC_FN void add_bin(Stats &s, u32 b, u32 h) {
    if (h == 0u) return;
    s.sum_d += (u64)b * h;
    s.sum_d2 += (u64)b * b * h;
    s.proc_win += h;
    if (b != 0u) s.cov_win += h;
    if (b < s.min_d) s.min_d = b;
    if (b > s.max_d) s.max_d = b;
}

// two disjoint sets of bins of one histogram
HSTC_FN void merge(Stats &s, const Stats &o) {
    s.sum_d += o.sum_d; s.sum_d2 += o.sum_d2; s.cov_win += o.cov_win; s.proc_win += o.proc_win;
    if (o.min_d < s.min_d) s.min_d = o.min_d;
    if (o.max_d > s.max_d) s.max_d = o.max_d;
}

// bins first, first + stride, ... below n  (first = 0, stride = 1: the whole histogram)
HSTC_FN Stats of_bins(const u32 *bins, u64 n, u32 first, u32 stride) {
    Stats s = empty();
    for (u64 b = first; b < n; b += stride) add_bin(s, (u32)b, bins[b]);
    return s;
}

}  // namespace hstc
