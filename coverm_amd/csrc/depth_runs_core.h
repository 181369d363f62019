// Depth runs (cov_depth_runs_*): the arithmetic of the run-length encoding of the per-base depth, written once, run two ways (the functors
// of csrc/depth_kernels.hip.h behind the shared device-wide scan; serially on the CPU in runs_cpu below, which tests/c/depth_runs_host.cpp
// runs against numpy).
//
//   layout        a chunk holds whole targets.  Target k of the chunk owns words_of(L_k) WORDS of four i32 depths each, from word woff[k]
//                 on: at least one word (an empty target has a word of its own, so every target starts at a different word), and the
//                 entries behind its last base up to the word's end hold PAD.  A word therefore never holds bases of two targets, every
//                 target starts at a 16-byte boundary, and the first base of a word is the first base of a target exactly when the
//                 word's bit in the start mask (one bit per word) is set.
//   plan_chunk    the targets one chunk takes under a budget of arena entries: at least one, then as many as still fit.
//   run_starts    the bases of one word that start a run: not PAD, and the first of its target or different from the base in front.
//   view          what the run arithmetic sees of an arena entry: the entry itself (Identity: runs of equal depth), or a function of it that
//                 keeps PAD (dclc::ClassView of csrc/depth_class_core.h: runs of equal depth class).  The start mask, rank and order are the same.
//   target_of     the chunk's target a word belongs to, from the start mask and the exclusive prefix of its popcounts (`rank`, one per
//                 32 words): the number of target starts at or in front of the word, less one.  No search over the offsets.
#pragma once
#include <stdint.h>

#ifndef DPRC_FN
#define DPRC_FN inline
#endif

namespace dprc {

typedef unsigned int u32;
typedef unsigned long long u64;

constexpr int32_t PAD = INT32_MIN;      // never a depth: depths are counts of reads
constexpr u64 DEFAULT_CHUNK_BASES = 1ull << 28;

struct Run { u32 start; int32_t depth; };      // cov_depth_run

DPRC_FN u32 words_of(u32 L) { return L == 0u ? 1u : (u32)(((u64)L + 3ull) >> 2); }

// First target behind the chunk that starts at `lo`: [lo, next) are the chunk's targets, lo < next <= hi (lo < hi).  `budget` counts arena
// entries (four per word); a target above the budget is a chunk of its own.
DPRC_FN u32 plan_chunk(const u32 *tlen, u32 lo, u32 hi, u64 budget) {
    u64 used = 4ull * words_of(tlen[lo]);
    u32 t = lo + 1u;
    while (t < hi) {
        const u64 e = 4ull * words_of(tlen[t]);
        if (used + e > budget) break;
        used += e; t++;
    }
    return t;
}

DPRC_FN u32 popc32(u32 x) {
    x = x - ((x >> 1) & 0x55555555u);
    x = (x & 0x33333333u) + ((x >> 2) & 0x33333333u);
    return (((x + (x >> 4)) & 0x0f0f0f0fu) * 0x01010101u) >> 24;
}

// bit j: base j of the word starts a run.  prev = the entry in front of the word (PAD for the arena's first word); tstart = the word's
// start-mask bit.
DPRC_FN u32 run_starts(int32_t d0, int32_t d1, int32_t d2, int32_t d3, int32_t prev, bool tstart) {
    return (u32)(d0 != PAD && (tstart || d0 != prev)) | (u32)(d1 != PAD && d1 != d0) << 1 | (u32)(d2 != PAD && d2 != d1) << 2 |
           (u32)(d3 != PAD && d3 != d2) << 3;
}

struct Identity { DPRC_FN int32_t operator()(int32_t d) const { return d; } };

DPRC_FN bool word_starts_target(const u32 *mask, u32 w) { return (mask[w >> 5] >> (w & 31u)) & 1u; }

DPRC_FN u32 target_of(const u32 *mask, const u32 *rank, u32 w) {
    return rank[w >> 5] + popc32(mask[w >> 5] & ((2u << (w & 31u)) - 1u)) - 1u;
}

// What the scan's functor returns for word w ...
template <class View = Identity>
DPRC_FN u32 count_word(const int32_t *arena, const u32 *mask, u32 w, const View &q = View()) {
    const int32_t *d = arena + 4ull * w;
    return popc32(run_starts(q(d[0]), q(d[1]), q(d[2]), q(d[3]), w ? q(d[-1]) : PAD, word_starts_target(mask, w)));
}
// ... and what its sink does with the word's exclusive prefix p: the word's runs go to runs[p ..], a target's first word leaves p in run_off.
template <class View = Identity>
DPRC_FN void emit_word(const int32_t *arena, const u32 *mask, const u32 *rank, const u32 *woff, u32 w, u32 p, Run *runs, u32 *run_off, const View &q = View()) {
    const int32_t d[4] = {q(arena[4ull * w]), q(arena[4ull * w + 1ull]), q(arena[4ull * w + 2ull]), q(arena[4ull * w + 3ull])};
    const bool ts = word_starts_target(mask, w);
    const u32 m = run_starts(d[0], d[1], d[2], d[3], w ? q(arena[4ull * w - 1ull]) : PAD, ts);
    if (!ts && !m) return;
    const u32 k = target_of(mask, rank, w);
    if (ts) run_off[k] = p;
    const u32 base = 4u * (w - woff[k]);
    for (u32 j = 0; j < 4u; j++)
        if (m >> j & 1u) { Run r; r.start = base + j; r.depth = d[j]; runs[p++] = r; }
}

// The chunk's layout: woff[0 .. n] from the lengths; returns the arena's words.
DPRC_FN u32 layout(const u32 *tlen, u32 n, u32 *woff) {
    u32 w = 0;
    for (u32 k = 0; k < n; k++) { woff[k] = w; w += words_of(tlen[k]); }
    woff[n] = w;
    return w;
}
// One target's marks: its start bit and the PAD entries behind its last base.  (The device sets the bit with an atomic OR: bits of one
// mask word belong to different targets; no order depends on it.)
DPRC_FN void mark_pads(int32_t *arena, const u32 *woff, const u32 *tlen, u32 k) {
    for (u64 e = 4ull * woff[k] + tlen[k], end = 4ull * woff[k + 1]; e < end; e++) arena[e] = PAD;
}

// The whole chunk serially, in the order of the device's launches: marks, rank scan, count, exclusive scan, emit.  arena: 4 * woff[n]
// entries holding the targets' depths at 4 * woff[k]; mask / rank: (words + 31) / 32 entries; run_off: n + 1; runs: as many as counted
// (runs == nullptr: only the count).  Returns the number of runs; a run's `depth` is the view's value.
template <class View = Identity>
DPRC_FN u64 runs_cpu(int32_t *arena, const u32 *tlen, u32 n, const u32 *woff, u32 *mask, u32 *rank, Run *runs, u32 *run_off, const View &q = View()) {
    const u32 words = woff[n], mw = (words + 31u) >> 5;
    for (u32 i = 0; i < mw; i++) mask[i] = 0u;
    for (u32 k = 0; k < n; k++) { mask[woff[k] >> 5] |= 1u << (woff[k] & 31u); mark_pads(arena, woff, tlen, k); }
    u32 r = 0;
    for (u32 i = 0; i < mw; i++) { rank[i] = r; r += popc32(mask[i]); }
    u64 total = 0;
    for (u32 w = 0; w < words; w++) {
        const u32 c = count_word(arena, mask, w, q);
        if (runs) emit_word(arena, mask, rank, woff, w, (u32)total, runs, run_off, q);
        total += c;
    }
    if (runs) run_off[n] = (u32)total;
    return total;
}

}  // namespace dprc
