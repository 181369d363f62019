// Depth bins (cov_depth_bins_*): the arithmetic of the reduction of the per-base depth over fixed windows, written once, run two ways (the
// kernels of csrc/depth_bins_kernels.hip.h; on the CPU in tests/c/depth_bins_host.cpp, against numpy's reduceat).  The chunk's layout, its
// start mask and rank are those of csrc/depth_runs_core.h.
//
//   geometry      target k of length L has bins_of(L, B) = ceil(L / B) bins of B bases, the last one short when B does not divide L; bins
//                 never cross a target boundary, an empty target has none.  The chunk's bins are numbered in target order, then position
//                 order: bin b of target k is the GLOBAL bin bin_off[k] + b, which never decreases along the arena.
//   word_partials what one lane does with one arena word (four i32 entries, PAD behind a target's last base): from the word's first
//                 position, B and the target's bin offset, the partial (bin, sum, min, max, covered) of every bin the word touches: one to
//                 four, ascending, all of one target; none for the all-PAD word of an empty target.  pos / B is computed once per word.
//   merge         a partial into a bin or into another partial of the same bin: add, min, max, add.  Commutative and associative on
//                 integers, so the order the partials arrive in cannot change a bit of the result.
#pragma once
#include <stdint.h>

#ifndef DBNC_FN
#define DBNC_FN inline
#endif
#ifndef DPRC_FN
#define DPRC_FN DBNC_FN
#endif
#include "depth_runs_core.h"
#if defined(__clang__)
#define DBNC_UNROLL _Pragma("unroll")
#else
#define DBNC_UNROLL
#endif

namespace dbnc {

using dprc::u32;
using dprc::u64;

constexpr u32 MAX_BIN_SIZE = 0x7fffffffu;
// A wave of the reduction owns a contiguous stretch of the arena: WAVE_STEPS loads of 64 words (1 KiB each).
constexpr u32 WAVE_STEPS = 16;
constexpr u32 STRETCH_WORDS = 64u * WAVE_STEPS;
constexpr u32 STRETCH_BASES = 4u * STRETCH_WORDS;      // the width of a wave's stretch in bases

struct Bin { u64 sum; int32_t min, max; u32 covered, reserved; };      // cov_depth_bin
struct Partial { u32 bin; int32_t min, max; u32 covered; u64 sum; };

// What a bin holds before its first base arrives, and what a word without a base contributes: merging it changes nothing.
DBNC_FN Partial identity(u32 bin) { Partial p; p.bin = bin; p.min = INT32_MAX; p.max = 0; p.covered = 0u; p.sum = 0ull; return p; }
DBNC_FN Bin empty_bin() { Bin b; b.sum = 0ull; b.min = INT32_MAX; b.max = 0; b.covered = 0u; b.reserved = 0u; return b; }

DBNC_FN u32 bins_of(u32 L, u32 B) { return L == 0u ? 0u : (L - 1u) / B + 1u; }
DBNC_FN u32 bin_len(u32 L, u32 B, u32 b) { const u64 lo = (u64)b * B, hi = lo + B; return (u32)((hi < L ? hi : (u64)L) - lo); }

// The chunk's bin offsets: bin_off[0 .. n] from the lengths; returns the chunk's bins.
DBNC_FN u64 bin_layout(const u32 *tlen, u32 n, u32 B, u64 *bin_off) {
    u64 b = 0;
    for (u32 k = 0; k < n; k++) { bin_off[k] = b; b += bins_of(tlen[k], B); }
    bin_off[n] = b;
    return b;
}

DBNC_FN void add_base(Partial &p, int32_t d) {
    p.sum += (u64)(u32)d;
    p.min = d < p.min ? d : p.min;
    p.max = d > p.max ? d : p.max;
    p.covered += d > 0 ? 1u : 0u;
}
DBNC_FN Partial merge(Partial a, const Partial &b) {      // (of the same bin)
    a.sum += b.sum;
    a.min = b.min < a.min ? b.min : a.min;
    a.max = b.max > a.max ? b.max : a.max;
    a.covered += b.covered;
    return a;
}
DBNC_FN void merge_into(Bin &dst, const Partial &p) {
    dst.sum += p.sum;
    dst.min = p.min < dst.min ? p.min : dst.min;
    dst.max = p.max > dst.max ? p.max : dst.max;
    dst.covered += p.covered;
}

// The partials of one word: d0 .. d3 its entries, pos0 = 4 * (w - woff[k]) its first position inside target k, bin0 = bin_off[k].
// Returns how many (0 .. 4); out[0 .. n) ascend by one in `bin`.  A bin strictly between out[0] and out[n - 1] lies wholly inside the word.
// (Every index into out[] and d[] is a constant once the loops are unrolled: on the device the partials stay in registers.)
DBNC_FN u32 word_partials(int32_t d0, int32_t d1, int32_t d2, int32_t d3, u32 pos0, u32 B, u32 bin0, Partial out[4]) {
    if (d0 == dprc::PAD) return 0u;
    const u32 q = pos0 / B, r = pos0 - q * B;      // r: bases of the word's first bin in front of the word
    const int32_t d[4] = {d0, d1, d2, d3};
    out[0] = identity(bin0 + q);
    if (B - r >= 4u) {      // the word lies in one bin (PAD only trails)
        DBNC_UNROLL
        for (u32 j = 0; j < 4u; j++)
            if (d[j] != dprc::PAD) add_base(out[0], d[j]);
        return 1u;
    }
    u32 idx[4], rr = r, c = 0u, n = 1u;      // idx[j]: the partial entry j belongs to
    idx[0] = 0u;
    DBNC_UNROLL
    for (u32 j = 1; j < 4u; j++) {
        if (++rr == B) { rr = 0u; c++; }
        idx[j] = c;
        if (d[j] != dprc::PAD) n = c + 1u;
    }
    DBNC_UNROLL
    for (u32 m = 0; m < 4u; m++) {
        out[m] = identity(bin0 + q + m);
        DBNC_UNROLL
        for (u32 j = 0; j < 4u; j++)
            if (d[j] != dprc::PAD && idx[j] == m) add_base(out[m], d[j]);
    }
    return n;
}

// One word of the arena as a lane sees it: its target from the start mask and rank, its partials.  `key` is the word's first bin, or, for
// a word without a base, the bin the next base of the chunk opens (bin_off of the empty target): the keys stay monotone along the arena,
// and merging identity() into that bin changes nothing.
DBNC_FN u32 word_of_arena(const int32_t *d, const u32 *mask, const u32 *rank, const u32 *woff, const u32 *bin_off, u32 w, u32 B, Partial out[4], u32 &key) {
    const u32 k = dprc::target_of(mask, rank, w);
    const u32 n = word_partials(d[0], d[1], d[2], d[3], 4u * (w - woff[k]), B, bin_off[k], out);
    key = n ? out[0].bin : bin_off[k];
    return n;
}

}  // namespace dbnc
