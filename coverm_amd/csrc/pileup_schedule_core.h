// How k_pileup_fast's tiles are handed to its waves.  Arithmetic only, no HIP: the kernel (pileup_kernels.hip.h, pileup_fast_body) and the
// host (covermhip.hip: the grid; tests/c/pileup_schedule_host.cpp: every wave's visits on the CPU) include the same rule.
//
// A launch has n_waves waves, n_tiles tiles cut into chunks of chunk_tiles consecutive tiles, and a list of n_deep tiles that k_ranges
// flagged TILE_F_DEEP (many candidate runs: an order of magnitude more work than a median tile, and neighbours of one another because they
// lie in the same few contigs).  Wave w visits
//     1. the list entries w, w + n_waves, ... below n_deep, ONE tile per visit, then
//     2. the chunks w, w + n_waves, ... below n_chunks, skipping the flagged tiles inside them.
// Low wave ids belong to the workgroups the dispatcher starts first, so the heavy tiles start first, spread one per wave over the whole
// device, and the light chunks fill in behind them.  Without a list (n_deep = 0) the sequence is the chunks alone.
#pragma once
#include <stdint.h>

#ifndef PSCHED_FN
#define PSCHED_FN inline
#endif

namespace psched {

typedef unsigned int u32;

// Grid of `wg_waves` waves per workgroup: PILEUP_ROUNDS x the resident waves, at most one wave per chunk.  The dispatcher hands the rounds
// out as workgroups retire, which evens out the heavy-tailed cost per chunk far better than a persistent grid of one round.  (16 and 32
// rounds were measured with the list in place and lost: profiles/pileup_schedule_ab.json.)
constexpr u32 PILEUP_ROUNDS = 8u;
// k_pileup_fast has no workgroup barrier and carves its LDS per wave: ONE wave per workgroup, so that a wave's slot is free the moment the
// wave is done and not when the slowest of four is.  (k_pileup_stream keeps four.)
constexpr u32 FAST_WG_WAVES = 1u, STREAM_WG_WAVES = 4u;
// tiles per chunk: with the deep tiles out of the chunks a chunk's cost no longer has a heavy tail, and longer chunks (fewer chunk ends,
// each of which moves the wave's bins) win; without a list the better balance of short chunks does
constexpr u32 CHUNK_TILES = 4u, CHUNK_TILES_LISTED = 8u;
constexpr u32 DEEP_MIN = 192u;      // candidate runs from which a tile goes on the list (COVERM_KNOBS pileup_deep_min)
PSCHED_FN u32 n_chunks_of(u32 n_tiles, u32 chunk_tiles) { return n_tiles / chunk_tiles + (n_tiles % chunk_tiles != 0u ? 1u : 0u); }
// workgroups of a launch; waves_per_cu = the waves of this kernel a CU holds
PSCHED_FN u32 grid_of(u32 n_tiles, u32 chunk_tiles, u32 n_cus, u32 waves_per_cu, u32 wg_waves) {
    const u32 nc = n_chunks_of(n_tiles, chunk_tiles), need = nc / wg_waves + (nc % wg_waves != 0u ? 1u : 0u), cap = n_cus * (waves_per_cu / wg_waves) * PILEUP_ROUNDS;
    const u32 g = need < cap ? need : cap;
    return g > 0u ? g : 1u;
}

struct Launch { u32 n_tiles, chunk_tiles, n_waves, n_deep, n_chunks; };
// (n_chunks costs an integer division: once per launch or wave here, never per visit)
PSCHED_FN Launch launch_of(u32 n_tiles, u32 chunk_tiles, u32 n_waves, u32 n_deep) {
    return Launch{n_tiles, chunk_tiles, n_waves, n_deep, n_chunks_of(n_tiles, chunk_tiles)};
}

// One visit of a wave: list entry `idx` (in_list) or chunk `idx`; done = the wave has nothing left.
struct Visit { u32 idx; bool in_list, done; };

PSCHED_FN Visit first_chunk(const Launch &L, u32 wave) {
    return Visit{wave, false, wave >= L.n_chunks};
}
PSCHED_FN Visit first(const Launch &L, u32 wave) {
    if (wave < L.n_deep) return Visit{wave, true, false};
    return first_chunk(L, wave);
}
// (idx + n_waves stays below 2^32 on any launch the host makes — idx < n_tiles, n_waves <= 2^22 —; a sum that wrapped ends the phase)
PSCHED_FN Visit next(const Launch &L, u32 wave, const Visit &v) {
    const u32 nx = v.idx + L.n_waves, end = v.in_list ? L.n_deep : L.n_chunks;
    if (nx < end && nx >= v.idx) return Visit{nx, v.in_list, false};
    if (v.in_list) return first_chunk(L, wave);
    return Visit{0u, false, true};
}
// tiles [t0, t1) of chunk ch
PSCHED_FN u32 chunk_t0(const Launch &L, u32 ch) { return ch * L.chunk_tiles; }
PSCHED_FN u32 chunk_t1(const Launch &L, u32 ch) {
    const u32 t0 = ch * L.chunk_tiles;
    return L.n_tiles - t0 < L.chunk_tiles ? L.n_tiles : t0 + L.chunk_tiles;
}

}  // namespace psched
