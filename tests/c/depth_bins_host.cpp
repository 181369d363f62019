// csrc/depth_bins_core.h on the CPU, as a program (tests/test_depth_bins_core.py; also built with -fsanitize=address,undefined).
// Input, one case after the other:
//   B  n  bin_size  seed  L_0 .. L_{n-1}   d ...      the bins of a chunk of n targets: their lengths, then sum(L) depths in target order
// The chunk is laid out as the device lays it out (dprc::layout / mark_pads, start mask, rank); the arena's words are then walked in an
// order shuffled by `seed` (0: ascending), each word's partials formed by dbnc::word_of_arena and merged into bins of dbnc::empty_bin().
// Output:
//   "N <bins> <arena words> <stretch bases>", "O bin_off_0 .. bin_off_n", "L len ..." (every bin's length), "S sum ...", "I min ...",
//   "A max ..." and "C covered ..."
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../../coverm_amd/csrc/depth_bins_core.h"

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: depth_bins_host <cases>\n"); return 2; }
    FILE *fh = fopen(argv[1], "r");
    if (!fh) { perror(argv[1]); return 2; }
    char kind[8];
    while (fscanf(fh, "%7s", kind) == 1) {
        unsigned n, B;
        unsigned long long seed;
        if (kind[0] != 'B' || fscanf(fh, "%u %u %llu", &n, &B, &seed) != 3 || B == 0 || B > dbnc::MAX_BIN_SIZE) return 3;
        std::vector<dbnc::u32> L(n), woff((size_t)n + 1);
        for (auto &x : L) if (fscanf(fh, "%u", &x) != 1) return 3;
        const dbnc::u32 words = dprc::layout(L.data(), n, woff.data()), mw = (words + 31u) >> 5;
        // exactly the sizes the headers promise to stay inside: the sanitized build sees any step outside them
        std::vector<int32_t> arena(4ull * words, 0);
        for (unsigned k = 0; k < n; k++)
            for (dbnc::u32 p = 0; p < L[k]; p++) if (fscanf(fh, "%d", &arena[4ull * woff[k] + p]) != 1) return 3;
        std::vector<dbnc::u32> mask(mw, 0u), rank(mw);
        for (unsigned k = 0; k < n; k++) { mask[woff[k] >> 5] |= 1u << (woff[k] & 31u); dprc::mark_pads(arena.data(), woff.data(), L.data(), k); }
        dbnc::u32 r = 0;
        for (dbnc::u32 i = 0; i < mw; i++) { rank[i] = r; r += dprc::popc32(mask[i]); }
        std::vector<dbnc::u64> bin_off((size_t)n + 1);
        const dbnc::u64 total = dbnc::bin_layout(L.data(), n, B, bin_off.data());
        if (total > 0xffffffffull) return 4;
        std::vector<dbnc::u32> bin_off32(bin_off.begin(), bin_off.end());
        std::vector<dbnc::Bin> bins(total, dbnc::empty_bin());
        std::vector<dbnc::u32> order(words);
        for (dbnc::u32 w = 0; w < words; w++) order[w] = w;
        dbnc::u64 x = seed;
        if (seed)
            for (dbnc::u32 i = words; i > 1u; i--) {      // Fisher-Yates over a 64-bit LCG
                x = x * 6364136223846793005ull + 1442695040888963407ull;
                std::swap(order[i - 1u], order[(x >> 33) % i]);
            }
        for (dbnc::u32 w : order) {
            dbnc::Partial P[4];
            dbnc::u32 key = 0;
            const dbnc::u32 np = dbnc::word_of_arena(arena.data() + 4ull * w, mask.data(), rank.data(), woff.data(), bin_off32.data(), w, B, P, key);
            if (np > 4u || key > total) return 5;
            for (dbnc::u32 j = 0; j < np; j++) {
                if (P[j].bin >= total || P[j].bin != P[0].bin + j || P[0].bin != key) return 6;
                dbnc::merge_into(bins[P[j].bin], P[j]);
            }
        }
        printf("N %llu %u %u\nO", total, words, dbnc::STRETCH_BASES);
        for (auto o : bin_off) printf(" %llu", o);
        printf("\nL");
        for (unsigned k = 0; k < n; k++)
            for (dbnc::u32 b = 0; b < dbnc::bins_of(L[k], B); b++) printf(" %u", dbnc::bin_len(L[k], B, b));
        printf("\nS");
        for (auto &b : bins) printf(" %llu", b.sum);
        printf("\nI");
        for (auto &b : bins) printf(" %d", b.min);
        printf("\nA");
        for (auto &b : bins) printf(" %d", b.max);
        printf("\nC");
        for (auto &b : bins) printf(" %u", b.covered);
        printf("\n");
    }
    fclose(fh);
    return 0;
}
