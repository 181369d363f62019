// csrc/depth_regions_core.h on the CPU, as a program (tests/test_depth_regions_core.py; also built with -fsanitize=address,undefined).
// Input, one case after the other:
//   G  n  m  seed  L_0 .. L_{n-1}   d ...   (k start end) x m
// a chunk of n targets: their lengths, then sum(L) depths in target order, then m regions [start, end) of target k in any order.
// The chunk is laid out as the device lays it out (dprc::layout / mark_pads); every region gets its descriptor from woff[], piece_off is the
// exclusive prefix of the regions' pieces.  The PIECES are then processed in an order shuffled by `seed` (0: ascending) the way a wave
// processes one: region_of_piece, the piece's words [piece_begin, piece_end) through drgc::add_word, lane by lane (word i goes to lane i % 64),
// the 64 lane partials merged, the piece merged into the region's dbnc::empty_bin() by merge_into.  Only words of the piece are read.
// region_of_piece is checked at both ends of every region's piece range.
// Output:
//   "N <regions> <pieces> <arena words> <stretch bases>", "P pieces ..." (per region), "S sum ...", "I min ...", "A max ...", "C covered ..."
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../../coverm_amd/csrc/depth_regions_core.h"

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: depth_regions_host <cases>\n"); return 2; }
    FILE *fh = fopen(argv[1], "r");
    if (!fh) { perror(argv[1]); return 2; }
    char kind[8];
    while (fscanf(fh, "%7s", kind) == 1) {
        unsigned n, m;
        unsigned long long seed;
        if (kind[0] != 'G' || fscanf(fh, "%u %u %llu", &n, &m, &seed) != 3) return 3;
        std::vector<drgc::u32> L(n), woff((size_t)n + 1);
        for (auto &x : L) if (fscanf(fh, "%u", &x) != 1) return 3;
        const drgc::u32 words = dprc::layout(L.data(), n, woff.data());
        // exactly the size the headers promise to stay inside: the sanitized build sees any step outside it
        std::vector<int32_t> arena(4ull * words, 0);
        for (unsigned k = 0; k < n; k++) {
            for (drgc::u32 p = 0; p < L[k]; p++) if (fscanf(fh, "%d", &arena[4ull * woff[k] + p]) != 1) return 3;
            dprc::mark_pads(arena.data(), woff.data(), L.data(), k);
        }
        std::vector<drgc::Desc> desc(m);
        for (unsigned r = 0; r < m; r++) {
            unsigned k, a, e;
            if (fscanf(fh, "%u %u %u", &k, &a, &e) != 3 || k >= n || a >= e || e > L[k]) return 3;
            desc[r] = drgc::describe(woff[k], a, e);
            if (drgc::pieces_of(desc[r]) != drgc::pieces_of_region(a, e) || desc[r].w_lo + desc[r].words > woff[k + 1]) return 4;
        }
        std::vector<drgc::u64> piece_off64((size_t)m + 1);
        const drgc::u64 total = drgc::piece_layout(desc.data(), m, piece_off64.data());
        if (total > 0xffffffffull) return 4;
        std::vector<drgc::u32> piece_off(piece_off64.begin(), piece_off64.end());
        for (unsigned r = 0; r < m; r++)      // every piece boundary
            if (drgc::region_of_piece(piece_off.data(), m, piece_off[r]) != r || drgc::region_of_piece(piece_off.data(), m, piece_off[r + 1] - 1u) != r) return 5;
        std::vector<drgc::Bin> out(m, dbnc::empty_bin());
        std::vector<drgc::u32> order((size_t)total);
        for (drgc::u32 p = 0; p < total; p++) order[p] = p;
        drgc::u64 x = seed;
        if (seed)
            for (drgc::u32 i = (drgc::u32)total; i > 1u; i--) {      // Fisher-Yates over a 64-bit LCG
                x = x * 6364136223846793005ull + 1442695040888963407ull;
                std::swap(order[i - 1u], order[(x >> 33) % i]);
            }
        for (drgc::u32 p : order) {
            const drgc::u32 r = drgc::region_of_piece(piece_off.data(), m, p);
            if (r >= m || p < piece_off[r] || p >= piece_off[r + 1]) return 5;
            const drgc::Desc &d = desc[r];
            const drgc::u32 q = p - piece_off[r], i0 = drgc::piece_begin(q), i1 = drgc::piece_end(d, q);
            if (i0 >= i1 || i1 - i0 > dbnc::STRETCH_WORDS || i1 > d.words) return 6;
            drgc::Partial lane[64];
            for (auto &P : lane) P = dbnc::identity(r);
            for (drgc::u32 i = i0; i < i1; i++) {
                const int32_t *w = arena.data() + 4ull * (d.w_lo + i);
                drgc::add_word(lane[(i - i0) & 63u], d, i, w[0], w[1], w[2], w[3]);
            }
            drgc::Partial P = lane[0];
            for (unsigned l = 1; l < 64; l++) P = dbnc::merge(P, lane[l]);
            dbnc::merge_into(out[r], P);
        }
        printf("N %u %llu %u %u\nP", m, total, words, dbnc::STRETCH_BASES);
        for (auto &d : desc) printf(" %u", drgc::pieces_of(d));
        printf("\nS");
        for (auto &b : out) printf(" %llu", b.sum);
        printf("\nI");
        for (auto &b : out) printf(" %d", b.min);
        printf("\nA");
        for (auto &b : out) printf(" %d", b.max);
        printf("\nC");
        for (auto &b : out) printf(" %u", b.covered);
        printf("\n");
    }
    fclose(fh);
    return 0;
}
