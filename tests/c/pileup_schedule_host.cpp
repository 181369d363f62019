// csrc/pileup_schedule_core.h on the CPU: for a grid of launches, every wave's visits are enumerated with the same first / next rule the
// kernel runs, and their union must cover every list entry exactly once and every unflagged tile exactly once, touch no flagged tile in
// the chunk phase, and produce no index past either end.  Built plainly and with -fsanitize=address,undefined (tests/test_pileup_schedule_core.py).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../coverm_amd/csrc/pileup_schedule_core.h"

using psched::u32;

static int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (failures < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
            failures++;                                   \
        }                                                 \
    } while (0)

// placement of the n_deep flagged tiles among n_tiles: 0 = at the front, 1 = at the back, 2 = scattered
static std::vector<u32> place(u32 n_tiles, u32 n_deep, int how) {
    std::vector<u32> list;
    if (how == 0) for (u32 i = 0; i < n_deep; i++) list.push_back(i);
    else if (how == 1) for (u32 i = 0; i < n_deep; i++) list.push_back(n_tiles - 1u - i);
    else {      // a stride coprime to n_tiles visits distinct tiles
        u32 stride = 7u;
        while (n_tiles % stride == 0u && stride < n_tiles) stride += 2u;
        if (n_tiles <= 7u) stride = 1u;
        for (u32 i = 0; i < n_deep; i++) list.push_back((u32)(((unsigned long long)i * stride + 3u) % n_tiles));
    }
    return list;
}

static void run_cell(u32 n_tiles, u32 chunk_tiles, u32 n_waves, u32 n_deep, int how) {
    const std::vector<u32> list = place(n_tiles, n_deep, how);
    std::vector<unsigned char> flagged(n_tiles, 0);
    for (u32 t : list) { CHECK(t < n_tiles && !flagged[t], "placement repeats tile %u", t); flagged[t] = 1; }
    std::vector<u32> list_seen(n_deep, 0), tile_seen(n_tiles, 0);
    const psched::Launch L = psched::launch_of(n_tiles, chunk_tiles, n_waves, n_deep);
    const u32 n_chunks = L.n_chunks;
    CHECK((unsigned long long)n_chunks * chunk_tiles >= n_tiles && (n_chunks == 0u || (unsigned long long)(n_chunks - 1u) * chunk_tiles < n_tiles), "n_chunks %u", n_chunks);
    for (u32 w = 0; w < n_waves; w++) {
        bool chunk_phase = false;
        unsigned long long visits = 0;
        for (psched::Visit v = psched::first(L, w); !v.done; v = psched::next(L, w, v)) {
            CHECK(++visits <= (unsigned long long)n_deep + n_chunks + 1u, "wave %u does not end", w);
            if (visits > (unsigned long long)n_deep + n_chunks + 1u) break;
            if (v.in_list) {
                CHECK(!chunk_phase, "wave %u returns to the list after a chunk", w);
                CHECK(v.idx < n_deep, "list index %u of %u", v.idx, n_deep);
                CHECK(v.idx % n_waves == w, "list index %u is not wave %u's", v.idx, w);
                if (v.idx < n_deep) {
                    list_seen[v.idx]++;
                    const u32 t = list[v.idx];      // (one tile per visit)
                    tile_seen[t]++;
                }
            } else {
                chunk_phase = true;
                CHECK(v.idx < n_chunks, "chunk %u of %u", v.idx, n_chunks);
                CHECK(v.idx % n_waves == w, "chunk %u is not wave %u's", v.idx, w);
                if (v.idx >= n_chunks) continue;
                const u32 t0 = psched::chunk_t0(L, v.idx), t1 = psched::chunk_t1(L, v.idx);
                CHECK(t0 < t1 && t1 <= n_tiles && t1 - t0 <= chunk_tiles, "chunk %u = [%u, %u) of %u tiles", v.idx, t0, t1, n_tiles);
                for (u32 t = t0; t < t1 && t < n_tiles; t++)
                    if (!flagged[t]) tile_seen[t]++;      // (the kernel skips TILE_F_DEEP tiles inside a chunk)
            }
        }
    }
    for (u32 i = 0; i < n_deep; i++) CHECK(list_seen[i] == 1u, "n_tiles %u chunk %u waves %u deep %u how %d: list entry %u visited %u times", n_tiles, chunk_tiles, n_waves, n_deep, how, i, list_seen[i]);
    for (u32 t = 0; t < n_tiles; t++) CHECK(tile_seen[t] == 1u, "n_tiles %u chunk %u waves %u deep %u how %d: tile %u (flagged %d) visited %u times", n_tiles, chunk_tiles, n_waves, n_deep, how, t, (int)flagged[t], tile_seen[t]);
}

int main() {
    const u32 tiles[] = {0u, 1u, 3u, 4u, 5u, 1000u}, chunks[] = {1u, 2u, 4u, 7u}, waves[] = {4u, 12u, 64u};
    unsigned cells = 0;
    for (u32 n_tiles : tiles)
        for (u32 ct : chunks)
            for (u32 nw : waves) {
                const u32 deeps[] = {0u, 1u, nw - 1u, nw, 3u * nw + 1u, n_tiles};
                for (u32 nd : deeps) {
                    if (nd > n_tiles) continue;      // (a list cannot hold more tiles than there are)
                    for (int how = 0; how < 3; how++) { run_cell(n_tiles, ct, nw, nd, how); cells++; }
                }
            }
    printf("cells: %u\n", cells);
    // the grid: at most a wave per chunk, at most PILEUP_ROUNDS rounds of the resident waves, never empty
    for (u32 wgw : {1u, 4u}) {
        CHECK(psched::grid_of(0u, 4u, 256u, 28u, wgw) == 1u, "empty grid");
        CHECK(psched::grid_of(1u, 4u, 256u, 28u, wgw) == 1u, "one tile");
        CHECK(psched::grid_of(17u, 4u, 256u, 28u, wgw) == (wgw == 1u ? 5u : 2u), "17 tiles = 5 chunks = 5 waves = 2 workgroups of four");
        CHECK(psched::grid_of(1u << 24, 4u, 256u, 28u, wgw) * wgw == 256u * 28u * psched::PILEUP_ROUNDS, "capped grid");
    }
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
