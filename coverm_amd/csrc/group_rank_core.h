// cov_group_records — records grouped by reference with a stable LSD radix sort of their indices: the arithmetic of one pass, written once,
// run two ways (the kernels in csrc/group_kernels.hip.h; lane by lane on the CPU in tests/c/group_rank_host.cpp against numpy's stable
// argsort).  Nothing here touches memory or the wave: the caller hands in ballots and counts, however it got them.
//
// Key of a record: its tid, or n_targets for a record without a reference (tid < 0; a tid at or beyond n_targets, which cov_finish reports
// as COV_ERR_BAD_TID, shares that key) — the order rec_key (ingest_kernels.hip.h) gives: references ascending, the rest last.  Digits of
// 8 bits, lowest first, only as many as n_targets needs.
//
// One pass over a workgroup's tile of TILE consecutive items (WAVES waves of 64 lanes, ITEMS rounds; in round r lane l of wave w holds
// item r * 256 + 64 w + l of the tile, so that "earlier in the tile" is "earlier round, then lower wave, then lower lane"):
//   rank of an item among the items of the whole input with its digit
//     = base[digit][workgroup]               items with a lower digit anywhere + items with this digit in earlier workgroups: the exclusive
//                                            scan over the workgroups' histograms laid out digit-major (hist_index)
//     + items with this digit in earlier rounds of the tile            `running`, kept per digit
//     + ... in lower waves of this round                               wave_bases over the waves' counts
//     + ... in lower lanes of this wave                                rank_among(peers_of(...), lane)
// Every term is a count, none is the outcome of a race: the permutation is the stable one and the same in every run.
#pragma once
#include <stdint.h>

#ifndef GRPK_FN
#define GRPK_FN inline
#endif

namespace grpk {

typedef unsigned int u32;
typedef unsigned long long u64;

constexpr u32 RADIX_BITS = 8u, RADIX = 1u << RADIX_BITS;
constexpr u32 WAVE = 64u, WAVES = 4u, WG = WAVE * WAVES;      // WG == RADIX: thread t of the workgroup also looks after digit t
constexpr u32 ITEMS = 16u, TILE = WG * ITEMS;
static_assert(WG == RADIX, "one thread per digit");

GRPK_FN u32 key_of(int32_t tid, u32 n_targets) { return (u32)tid < n_targets ? (u32)tid : n_targets; }
// passes that distinguish the keys 0 .. n_targets: ceil(log2(n_targets + 1)) bits in digits of 8 (at least one)
GRPK_FN u32 n_passes(u32 n_targets) {
    u32 p = 1u;
    while (p < 4u && (n_targets >> (RADIX_BITS * p)) != 0u) p++;
    return p;
}
GRPK_FN u32 digit_of(u32 key, u32 pass) { return (key >> (RADIX_BITS * pass)) & (RADIX - 1u); }
GRPK_FN u32 n_tiles(u64 n) { return (u32)((n + TILE - 1u) / TILE); }
// where workgroup wg's count of digit d lies: digit-major, so that ONE exclusive scan over the array yields base[d][wg]
GRPK_FN u64 hist_index(u32 d, u32 wg, u32 n_wg) { return (u64)d * n_wg + wg; }

GRPK_FN u32 popc(u64 m) { return (u32)__builtin_popcountll(m); }
// One bit of the digit folded into the peers mask: `ballot` = the lanes whose digit has bit b set.  Start from the ballot of the lanes
// that hold an item; after RADIX_BITS steps the mask holds exactly the item-holding lanes whose digit equals `digit`.
GRPK_FN u64 peers_step(u64 m, u32 digit, u32 b, u64 ballot) { return m & (((digit >> b) & 1u) ? ballot : ~ballot); }
GRPK_FN u32 rank_among(u64 peers, u32 lane) { return popc(peers & ((1ull << lane) - 1ull)); }
GRPK_FN bool is_leader(u64 peers, u32 lane) { return (peers & ((1ull << lane) - 1ull)) == 0ull; }      // lowest lane of its peers: it posts the wave's count

// The digit's thread, once per round: cnt[w] = the count wave w posted for this digit (0 if none); out[w] = where wave w's first such item
// goes; returns the digit's new `running`.
GRPK_FN u32 wave_bases(u32 running, const u32 cnt[WAVES], u32 out[WAVES]) {
    for (u32 w = 0; w < WAVES; w++) { out[w] = running; running += cnt[w]; }
    return running;
}

}  // namespace grpk
