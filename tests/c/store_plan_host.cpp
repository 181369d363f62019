// Host instantiation of csrc/store_plan_core.h beside the two first-window formulas the ingests carried before they shared one (frozen here,
// written out as they stood in ingest_drain_ and cov_sam_feed).  Test infrastructure (tests/test_store_plan_core.py builds it with g++, as
// a library for the comparisons and as a program — main below walks the same grid — for a run under the sanitizers); not part of the product.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>

#include "../../coverm_amd/csrc/store_plan_core.h"

typedef unsigned long long u64;

// ingest_drain_ (BGZF): enlarge, then bound by the cap without going below what the window needs
static u64 frozen_bgzf(u64 have, u64 add, u64 spare, double scale, u64 cap) {
    u64 Nn = have + add + spare;
    Nn = std::max<u64>(Nn, have + (u64)((double)add * scale) + 1024);
    Nn = std::max<u64>(have + add + spare, std::min<u64>(Nn, std::min<u64>(cap + 1024, 0xfffffff0ull)));
    return Nn;
}
// cov_sam_feed: the enlarged size bounded by the cap, if that is more than the window needs
static u64 frozen_sam(u64 have, u64 add, u64 spare, double scale, u64 cap) {
    u64 Nn = have + add + spare;
    Nn = std::max<u64>(Nn, std::min<u64>(have + (u64)((double)add * scale) + 1024, std::min<u64>(cap + 1024, 0xfffffff0ull)));
    return Nn;
}

extern "C" {
uint64_t stplan_size(uint64_t have, uint64_t add, uint64_t spare, double scale, uint64_t cap) { return stplan::first_window_size(have, add, spare, scale, cap); }
uint64_t stplan_size_frozen_bgzf(uint64_t have, uint64_t add, uint64_t spare, double scale, uint64_t cap) { return frozen_bgzf(have, add, spare, scale, cap); }
uint64_t stplan_size_frozen_sam(uint64_t have, uint64_t add, uint64_t spare, double scale, uint64_t cap) { return frozen_sam(have, add, spare, scale, cap); }
int stplan_spill_first(int store_empty, int mates_wanted, int failure_pending, int over_records, int over_cigar) {
    return stplan::spill_first(store_empty != 0, mates_wanted != 0, failure_pending != 0, over_records != 0, over_cigar != 0) ? 1 : 0;
}
int stplan_past_limit(uint64_t have, uint64_t add) { return stplan::past_limit(have, add) ? 1 : 0; }
}

int main() {
    const u64 caps[] = {50000ull, 1ull << 31, 1ull << 32};
    const double scales[] = {1.0001, 1.1, 7.3, 1e6};
    u64 n = 0, bad = 0;
    for (u64 cap : caps) {
        const u64 haves[] = {0, 1, cap - 1, cap, (1ull << 32) - 17};
        const u64 adds[] = {1, 1000, cap};
        for (u64 have : haves) for (u64 add : adds) for (double scale : scales) for (u64 spare = 0; spare < 2; spare++, n++) {
            const u64 got = stplan::first_window_size(have, add, spare, scale, cap), need = have + add + spare;
            if (got != frozen_bgzf(have, add, spare, scale, cap) || got != frozen_sam(have, add, spare, scale, cap)) bad++;
            if (got < need || got > std::max<u64>(need, std::min<u64>(cap + 1024, 0xfffffff0ull))) bad++;
        }
    }
    for (int b = 0; b < 32; b++, n++) {
        const bool empty = b & 1, mates = b & 2, fail = b & 4, over_r = b & 8, over_c = b & 16;
        if (stplan::spill_first(empty, mates, fail, over_r, over_c) != (!fail && !empty && !mates && (over_r || over_c))) bad++;
    }
    printf("%llu cases, %llu bad\n", n, bad);
    return bad ? 1 : 0;
}
