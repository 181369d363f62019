// csrc/hist_stats_core.h on the CPU, as a program (tests/test_hist_stats_core.py; also built with -fsanitize=address,undefined).
// The window statistics read off a depth histogram — by one walk over all bins, and by 64 strided walks merged, as a wave does it —
// against a brute-force loop over the positions the histogram stands for (where it is too long for that: over the bins, in 128 bits).
// No input.  Prints one line per case group and "ok"; exit status 1 at the first difference.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../coverm_amd/csrc/hist_stats_core.h"

using hstc::Stats;
using hstc::u32;
using hstc::u64;

static bool same(const Stats &a, const Stats &b) {
    return a.sum_d == b.sum_d && a.sum_d2 == b.sum_d2 && a.cov_win == b.cov_win && a.proc_win == b.proc_win && a.min_d == b.min_d && a.max_d == b.max_d;
}
static void show(const char *what, const Stats &s) {
    fprintf(stderr, "  %s: sum_d %llu sum_d2 %llu cov_win %llu proc_win %llu min_d %u max_d %u\n", what, s.sum_d, s.sum_d2, s.cov_win, s.proc_win, s.min_d, s.max_d);
}

// what the pileup kernels sum per position: `sum_d += d; sum_d2 += (u64)d * d; ...` for every position at depth d
static Stats per_position(const std::vector<u32> &bins) {
    Stats s{0, 0, 0, 0, 0xffffffffu, 0};
    for (size_t d = 0; d < bins.size(); d++)
        for (u32 k = 0; k < bins[d]; k++) {
            const u32 du = (u32)d;
            s.sum_d += du; s.sum_d2 += (u64)du * du; s.cov_win += du != 0u; s.proc_win++;
            if (du < s.min_d) s.min_d = du;
            if (du > s.max_d) s.max_d = du;
        }
    return s;
}
// the same per bin in 128 bits, reduced modulo 2^64 at the end (for histograms too long to replay position by position)
static Stats per_bin_wide(const std::vector<u32> &bins) {
    unsigned __int128 s1 = 0, s2 = 0;
    Stats s{0, 0, 0, 0, 0xffffffffu, 0};
    for (size_t d = 0; d < bins.size(); d++) {
        if (!bins[d]) continue;
        s1 += (unsigned __int128)d * bins[d]; s2 += (unsigned __int128)d * d * bins[d];
        s.proc_win += bins[d]; if (d) s.cov_win += bins[d];
        if ((u32)d < s.min_d) s.min_d = (u32)d;
        if ((u32)d > s.max_d) s.max_d = (u32)d;
    }
    s.sum_d = (u64)s1; s.sum_d2 = (u64)s2;
    return s;
}

static int check(const char *name, const std::vector<u32> &bins, const Stats &want) {
    // exactly bins.size() words behind the pointer: the sanitized build sees any read outside them
    const Stats whole = hstc::of_bins(bins.data(), bins.size(), 0u, 1u);
    Stats merged = hstc::empty();
    for (u32 lane = 0; lane < 64u; lane++) hstc::merge(merged, hstc::of_bins(bins.data(), bins.size(), lane, 64u));
    if (same(whole, want) && same(merged, want)) return 0;
    fprintf(stderr, "%s: %zu bins differ\n", name, bins.size());
    show("want", want); show("whole", whole); show("merged", merged);
    return 1;
}

static u64 rng_state = 0x9e3779b97f4a7c15ull;
static u32 rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (u32)(rng_state >> 32); }

int main() {
    int bad = 0;
    // by construction
    bad += check("no bins", {}, Stats{0, 0, 0, 0, 0xffffffffu, 0});
    bad += check("empty histogram", std::vector<u32>(700, 0u), Stats{0, 0, 0, 0, 0xffffffffu, 0});
    bad += check("bin 0 only", {1234u, 0u, 0u}, Stats{0, 0, 0, 1234, 0, 0});
    {
        std::vector<u32> h(1, 7u);
        bad += check("single bin at 0", h, Stats{0, 0, 0, 7, 0, 0});
        h.assign(512, 0u); h[511] = 3u;
        bad += check("single bin at 511", h, Stats{3ull * 511, 3ull * 511 * 511, 3, 3, 511, 511});
        h.assign(513, 0u); h[512] = 5u;
        bad += check("single bin at 512", h, Stats{5ull * 512, 5ull * 512 * 512, 5, 5, 512, 512});
    }
    {
        // sum of b^2 H passes 2^64: 100 000^2 x (2^32 - 1) = 4.3e19 > 1.8e19 in one bin, and again over twenty; a per-position `+=` in 64 bits
        // is the 128-bit sum modulo 2^64
        std::vector<u32> h(100001, 0u);
        h[100000] = 0xffffffffu; h[2] = 9u;
        if (!(((unsigned __int128)100000 * 100000 * 0xffffffffu) >> 64)) { fprintf(stderr, "the wrap case does not wrap\n"); bad++; }
        bad += check("sum of squares passes 2^64", h, per_bin_wide(h));
        for (u32 b = 99980; b < 100000; b++) h[b] = 0xfffffff0u + (b & 15u);
        bad += check("sum of squares passes 2^64 several times", h, per_bin_wide(h));
        // and the two references agree where both can run
        std::vector<u32> g(300, 0u);
        g[0] = 5u; g[17] = 100000u; g[299] = 70000u;
        if (!same(per_position(g), per_bin_wide(g))) { fprintf(stderr, "the two references differ\n"); bad++; }
    }
    printf("constructed: %s\n", bad ? "FAILED" : "ok");
    // random histograms, replayed position by position
    int rbad = 0;
    for (int it = 0; it < 400; it++) {
        const u32 n = rnd() % 700u;                     // on both sides of the 64-lane stride and of the 512 LDS bins
        std::vector<u32> h(n, 0u);
        const u32 fill = rnd() % 4u;                    // 0: sparse, 1: half, 2: dense, 3: one bin
        for (u32 b = 0; b < n; b++) {
            const u32 r = rnd();
            if (fill == 2u || (fill == 1u && (r & 1u)) || (fill == 0u && (r & 31u) == 0u)) h[b] = (rnd() % 3000u) + ((r >> 8) % 5u == 0u ? 0u : 1u);
        }
        if (fill == 3u && n) h[rnd() % n] = rnd() % 100000u;
        rbad += check("random", h, per_position(h));
    }
    // random histograms with counts up to 2^32 - 1 (too long to replay: the 128-bit per-bin sums)
    for (int it = 0; it < 200; it++) {
        const u32 n = 1u + rnd() % 300u;
        std::vector<u32> h(n);
        for (u32 b = 0; b < n; b++) h[b] = (rnd() & 3u) ? rnd() : 0u;
        rbad += check("random wide", h, per_bin_wide(h));
    }
    printf("random: %s\n", rbad ? "FAILED" : "ok");
    bad += rbad;
    if (bad) return 1;
    printf("ok\n");
    return 0;
}
