// csrc/depth_class_core.h on the CPU, as a program (tests/test_depth_classes_core.py; also built with -fsanitize=address,undefined).
// Input, one case after the other:
//   V  n  c_0 .. c_{n-1}                                  the validator over a list of n values (n may be 0 or above 16)
//   C  n  c_0 .. c_{n-1}  m  d_0 .. d_{m-1}               class_of of m depths under a (valid) cut list
//   Q  n  c ...  t  L_0 .. L_{t-1}  d ...                 the quantised runs of a chunk of t targets (dprc::runs_cpu behind dclc::ClassView)
//   T  n  c ...  t  m  seed  L_0 .. L_{t-1}  d ...  (k start end) x m
//                                                         the threshold counts of m regions, the pieces merged in an order shuffled by seed
// Output:
//   V: "V ok" or "V <index> <what>"
//   C: "C class ..."
//   Q: "N <runs> <arena words>", "O run_off ...", "S start ...", "D class ..."
//   T: "K <regions> <thresholds>", then per region "T count ..."
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../../coverm_amd/csrc/depth_class_core.h"

static bool read_cuts(FILE *fh, std::vector<int32_t> &c) {
    unsigned n;
    if (fscanf(fh, "%u", &n) != 1) return false;
    c.resize(n);
    for (auto &x : c) { long long v; if (fscanf(fh, "%lld", &v) != 1) return false; x = (int32_t)v; }
    return true;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: depth_classes_host <cases>\n"); return 2; }
    FILE *fh = fopen(argv[1], "r");
    if (!fh) { perror(argv[1]); return 2; }
    char kind[8];
    while (fscanf(fh, "%7s", kind) == 1) {
        std::vector<int32_t> cuts;
        if (!read_cuts(fh, cuts)) return 3;
        dclc::u32 at = 0;
        const char *what = dclc::validate(cuts.data(), (dclc::u32)cuts.size(), &at);
        if (kind[0] == 'V') {
            if (what) printf("V %u %s\n", at, what); else printf("V ok\n");
            continue;
        }
        if (what) return 4;
        const dclc::Cuts C = dclc::make(cuts.data(), (dclc::u32)cuts.size());
        if (kind[0] == 'C') {
            unsigned m;
            if (fscanf(fh, "%u", &m) != 1) return 3;
            printf("C");
            for (unsigned i = 0; i < m; i++) {
                int32_t d;
                if (fscanf(fh, "%d", &d) != 1) return 3;
                printf(" %u", dclc::class_of(d, C));
            }
            printf("\n");
            continue;
        }
        unsigned n, m = 0;
        unsigned long long seed = 0;
        if (fscanf(fh, "%u", &n) != 1) return 3;
        if (kind[0] == 'T' && fscanf(fh, "%u %llu", &m, &seed) != 2) return 3;
        std::vector<dclc::u32> L(n), woff((size_t)n + 1);
        for (auto &x : L) if (fscanf(fh, "%u", &x) != 1) return 3;
        const dclc::u32 words = dprc::layout(L.data(), n, woff.data()), mw = (words + 31u) >> 5;
        // exactly the sizes the headers promise to stay inside: the sanitized build sees any step outside them
        std::vector<int32_t> arena(4ull * words, 0);
        for (unsigned k = 0; k < n; k++) {
            for (dclc::u32 p = 0; p < L[k]; p++) if (fscanf(fh, "%d", &arena[4ull * woff[k] + p]) != 1) return 3;
            dprc::mark_pads(arena.data(), woff.data(), L.data(), k);
        }
        if (kind[0] == 'Q') {
            const dclc::ClassView view{C};
            std::vector<dclc::u32> mask(mw), rank(mw), run_off((size_t)n + 1);
            const dclc::u64 total = dprc::runs_cpu(arena.data(), L.data(), n, woff.data(), mask.data(), rank.data(), (dprc::Run *)nullptr, (dclc::u32 *)nullptr, view);
            std::vector<dprc::Run> runs(total);
            if (dprc::runs_cpu(arena.data(), L.data(), n, woff.data(), mask.data(), rank.data(), runs.data(), run_off.data(), view) != total) return 4;
            printf("N %llu %u\nO", total, words);
            for (auto o : run_off) printf(" %u", o);
            printf("\nS");
            for (auto &r : runs) printf(" %u", r.start);
            printf("\nD");
            for (auto &r : runs) printf(" %d", r.depth);
            printf("\n");
            continue;
        }
        if (kind[0] != 'T') return 3;
        // the pieces of the regions as a wave takes them (tests/c/depth_regions_host.cpp), counting instead of reducing
        std::vector<drgc::Desc> desc(m);
        for (unsigned r = 0; r < m; r++) {
            unsigned k, a, e;
            if (fscanf(fh, "%u %u %u", &k, &a, &e) != 3 || k >= n || a >= e || e > L[k]) return 3;
            desc[r] = drgc::describe(woff[k], a, e);
        }
        std::vector<dclc::u64> piece_off64((size_t)m + 1);
        const dclc::u64 total = drgc::piece_layout(desc.data(), m, piece_off64.data());
        if (total > 0xffffffffull) return 4;
        std::vector<dclc::u32> piece_off(piece_off64.begin(), piece_off64.end());
        std::vector<dclc::u32> order((size_t)total), counts((size_t)m * C.n, 0u);
        for (dclc::u32 p = 0; p < total; p++) order[p] = p;
        dclc::u64 x = seed;
        if (seed)
            for (dclc::u32 i = (dclc::u32)total; i > 1u; i--) {      // Fisher-Yates over a 64-bit LCG
                x = x * 6364136223846793005ull + 1442695040888963407ull;
                std::swap(order[i - 1u], order[(x >> 33) % i]);
            }
        for (dclc::u32 p : order) {
            const dclc::u32 r = drgc::region_of_piece(piece_off.data(), m, p);
            const drgc::Desc &d = desc[r];
            const dclc::u32 q = p - piece_off[r], i0 = drgc::piece_begin(q), i1 = drgc::piece_end(d, q);
            dclc::u32 lane[64][dclc::MAX_CUTS] = {};
            for (dclc::u32 i = i0; i < i1; i++) {
                const int32_t *w = arena.data() + 4ull * (d.w_lo + i);
                int32_t e[4] = {w[0], w[1], w[2], w[3]};
                dclc::mask_word(d, i, e);
                dclc::count_word(C, e, lane[(i - i0) & 63u]);
            }
            for (unsigned l = 0; l < 64; l++)
                for (dclc::u32 t = 0; t < C.n; t++) counts[(size_t)r * C.n + t] += lane[l][t];
        }
        printf("K %u %u\n", m, C.n);
        for (unsigned r = 0; r < m; r++) {
            printf("T");
            for (dclc::u32 t = 0; t < C.n; t++) printf(" %u", counts[(size_t)r * C.n + t]);
            printf("\n");
        }
    }
    fclose(fh);
    return 0;
}
