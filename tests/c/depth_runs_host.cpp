// csrc/depth_runs_core.h on the CPU, as a program (tests/test_depth_runs_core.py; also built with -fsanitize=address,undefined).
// Input, one case after the other:
//   R  n  L_0 .. L_{n-1}   d ...        the runs of a chunk of n targets: their lengths, then sum(L) depths in target order
//   P  n  budget  L_0 .. L_{n-1}        the planner over targets [0, n)
// Output:
//   R: "N <runs> <arena words>", "O run_off_0 .. run_off_n", "S start ..." and "D depth ..."
//   P: "P next_0 next_1 ..." — the first target behind every chunk, the last one is n
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../coverm_amd/csrc/depth_runs_core.h"

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: depth_runs_host <cases>\n"); return 2; }
    FILE *fh = fopen(argv[1], "r");
    if (!fh) { perror(argv[1]); return 2; }
    char kind[8];
    while (fscanf(fh, "%7s", kind) == 1) {
        unsigned n;
        if (fscanf(fh, "%u", &n) != 1) return 3;
        if (kind[0] == 'P') {
            unsigned long long budget;
            if (fscanf(fh, "%llu", &budget) != 1) return 3;
            std::vector<dprc::u32> L(n);
            for (auto &x : L) if (fscanf(fh, "%u", &x) != 1) return 3;
            printf("P");
            for (dprc::u32 lo = 0; lo < n;) { lo = dprc::plan_chunk(L.data(), lo, n, budget); printf(" %u", lo); }
            printf("\n");
            continue;
        }
        std::vector<dprc::u32> L(n), woff((size_t)n + 1);
        for (auto &x : L) if (fscanf(fh, "%u", &x) != 1) return 3;
        const dprc::u32 words = dprc::layout(L.data(), n, woff.data()), mw = (words + 31u) >> 5;
        // exactly the sizes the header promises to stay inside: the sanitized build sees any step outside them
        std::vector<int32_t> arena(4ull * words, 0);
        for (unsigned k = 0; k < n; k++)
            for (dprc::u32 p = 0; p < L[k]; p++) if (fscanf(fh, "%d", &arena[4ull * woff[k] + p]) != 1) return 3;
        std::vector<dprc::u32> mask(mw), rank(mw), run_off((size_t)n + 1);
        const dprc::u64 total = dprc::runs_cpu(arena.data(), L.data(), n, woff.data(), mask.data(), rank.data(), nullptr, nullptr);
        std::vector<dprc::Run> runs(total);
        if (dprc::runs_cpu(arena.data(), L.data(), n, woff.data(), mask.data(), rank.data(), runs.data(), run_off.data()) != total) return 4;
        printf("N %llu %u\nO", total, words);
        for (auto o : run_off) printf(" %u", o);
        printf("\nS");
        for (auto &r : runs) printf(" %u", r.start);
        printf("\nD");
        for (auto &r : runs) printf(" %d", r.depth);
        printf("\n");
    }
    fclose(fh);
    return 0;
}
