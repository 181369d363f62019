// Depth regions (cov_depth_regions_*): the arithmetic of the reduction of the per-base depth over arbitrary [start, end) intervals of a BED
// file, written once, run two ways (the kernel of csrc/depth_regions_kernels.hip.h; on the CPU in tests/c/depth_regions_host.cpp, against
// numpy slices).  The chunk's layout is that of csrc/depth_runs_core.h, the partial and its merge are those of csrc/depth_bins_core.h.
//
//   region        [start, end) of target tid, 0-based, half open, start < end <= length(tid): it never holds a PAD entry.  Regions may
//                 overlap, repeat and come in any order; each is reduced on its own.
//   descriptor    what the device sees of a region, built on the host from the chunk's woff[]: w_lo = woff[k] + start / 4 its first arena
//                 word, skip = start % 4 the entries of that word in front of the region, len = end - start, words = ceil((skip + len) / 4)
//                 the words it touches (w_lo .. w_lo + words - 1).  No target lookup, no mask and no rank on the device.
//   pieces        a region is cut into pieces of at most dbnc::STRETCH_WORDS words, counted from w_lo: pieces_of = ceil(words /
//                 STRETCH_WORDS); piece_off[0 .. n] is the exclusive prefix over the chunk's regions (every region has a piece, so it
//                 strictly increases) and region_of_piece the upper_bound - 1 over it: one wave takes one piece.
//   word          entry j of the region's word i is the region-relative base 4 i + j - skip; it counts iff 0 <= base < len.  What lies
//                 outside (the `skip` entries in front, the entries behind the last base, which may be a neighbour's depth or PAD) is
//                 never added.
//   merge         dbnc::merge / merge_into: integers, commutative and associative, so the order the pieces arrive in cannot change a bit.
#pragma once
#include <stdint.h>

#ifndef DRGC_FN
#define DRGC_FN inline
#endif
#ifndef DBNC_FN
#define DBNC_FN DRGC_FN
#endif
#include "depth_bins_core.h"

namespace drgc {

using dprc::u32;
using dprc::u64;
using dbnc::Bin;
using dbnc::Partial;

struct Region { u32 tid, start, end, reserved; };      // cov_depth_region
struct Desc { u32 w_lo, skip, len, words; };           // 16 bytes: one scalar load of four dwords

// The descriptor of [start, end) in a target whose first arena word is `woff_k`.
DRGC_FN Desc describe(u32 woff_k, u32 start, u32 end) {
    Desc d;
    d.w_lo = woff_k + (start >> 2); d.skip = start & 3u; d.len = end - start;
    d.words = (u32)(((u64)d.skip + d.len + 3ull) >> 2);
    return d;
}
DRGC_FN u32 pieces_of_words(u32 words) { return (words + dbnc::STRETCH_WORDS - 1u) / dbnc::STRETCH_WORDS; }
DRGC_FN u32 pieces_of(const Desc &d) { return pieces_of_words(d.words); }
// (before a chunk's layout is known: the pieces depend on the region alone)
DRGC_FN u32 pieces_of_region(u32 start, u32 end) { return pieces_of_words((u32)(((u64)(start & 3u) + (end - start) + 3ull) >> 2)); }

// piece_off[0 .. n] from the descriptors; returns the chunk's pieces (the caller refuses 2^32 or more before it narrows them to u32).
DRGC_FN u64 piece_layout(const Desc *desc, u32 n, u64 *piece_off) {
    u64 p = 0;
    for (u32 r = 0; r < n; r++) { piece_off[r] = p; p += pieces_of(desc[r]); }
    piece_off[n] = p;
    return p;
}

// The region piece p belongs to: the last r in [0, n) with piece_off[r] <= p (p < piece_off[n], n >= 1).  The same for every lane of a
// wave: on the device the loop runs in scalar registers.
DRGC_FN u32 region_of_piece(const u32 *piece_off, u32 n, u32 p) {
    u32 lo = 0u, hi = n;      // piece_off[lo] <= p < piece_off[hi]
    while (hi - lo > 1u) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (piece_off[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}

// One word of a region as a lane sees it: i = the word's index inside the region (0 .. words - 1), d0 .. d3 its entries.
DRGC_FN void add_word(Partial &P, const Desc &d, u32 i, int32_t d0, int32_t d1, int32_t d2, int32_t d3) {
    const int32_t e[4] = {d0, d1, d2, d3};
    const u32 b0 = 4u * i - d.skip;      // entry 0's base; in front of the region it wraps to 2^32 - skip .. 2^32 - 1, above every len
    // Every entry goes through add_base and a select keeps or drops the outcome: no branch per entry, so the four entries stay ONE 16-byte
    // load on the device (a branch around each entry's use lets the compiler split the load into four conditional ones).
    DBNC_UNROLL
    for (u32 j = 0; j < 4u; j++) {
        const bool in = b0 + j < d.len;
        Partial T = P;
        dbnc::add_base(T, e[j]);
        P.sum = in ? T.sum : P.sum; P.min = in ? T.min : P.min; P.max = in ? T.max : P.max; P.covered = in ? T.covered : P.covered;
    }
}

// The words [i0, i1) of piece q of a region: i0 = q * STRETCH_WORDS, i1 = min(words, i0 + STRETCH_WORDS).
DRGC_FN u32 piece_begin(u32 q) { return q * dbnc::STRETCH_WORDS; }
DRGC_FN u32 piece_end(const Desc &d, u32 q) { const u64 e = (u64)q * dbnc::STRETCH_WORDS + dbnc::STRETCH_WORDS; return e < d.words ? (u32)e : d.words; }

}  // namespace drgc
