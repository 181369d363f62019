// Depth classes (cov_depth_class_runs_compute, cov_depth_thresholds_set): a depth classified against a short ascending list of cut points,
// written once, run two ways (the functors of csrc/depth_kernels.hip.h and the threshold variant of csrc/depth_regions_kernels.hip.h; on the
// CPU in tests/c/depth_classes_host.cpp, against numpy's searchsorted and slices).
//
//   cut list      n values, 1 <= n <= MAX_CUTS, each in [0, 2^31 - 1], strictly ascending.  `validate` serves the quantised runs and the
//                 thresholds alike and names the first offending index.
//   class_of      the number of cuts c with c <= d: 0 (below the first cut) .. n (at or above the last).  The loop runs to n, never over
//                 padded slots: a sentinel in an unused slot would misclassify a depth of 2^31 - 1.  On the device the list travels by value
//                 in the kernel arguments (scalar registers), n is the same in every lane, and the loop is unrolled over MAX_CUTS with a
//                 uniform exit, so every index into the list is a constant: nothing is indexed at run time, nothing goes to scratch memory.
//   ClassView     what the run functors of csrc/depth_runs_core.h see of an arena entry: PAD stays PAD, a depth becomes its class.  Runs of
//                 equal class are then the runs of equal depth of the viewed arena: same start mask, same rank, same order.
//   thresholds    per region and threshold t, the bases with depth >= t.  `mask_word` turns the entries of a word that lie outside the region
//                 (drgc::add_word's test) into PAD, which is below every threshold: what is left is one compare per entry and threshold.
#pragma once
#include <stdint.h>

#ifndef DCLC_FN
#define DCLC_FN inline
#endif
#ifndef DRGC_FN
#define DRGC_FN DCLC_FN
#endif
#include "depth_regions_core.h"

namespace dclc {

using dprc::u32;
using dprc::u64;

constexpr u32 MAX_CUTS = 16;      // COV_DEPTH_MAX_CUTS

struct Cuts { int32_t c[MAX_CUTS]; u32 n; };      // unused slots hold 0 and are never read

// 0: the list is good.  Otherwise `at` is the first offending index and the return value says what is wrong with it.
DCLC_FN const char *validate(const int32_t *cuts, u32 n, u32 *at) {
    if (n == 0u) { *at = 0u; return "the list is empty (1 .. 16 values)"; }
    if (n > MAX_CUTS) { *at = MAX_CUTS; return "more than 16 values"; }
    for (u32 i = 0; i < n; i++) {
        if (cuts[i] < 0) { *at = i; return "a negative value (0 .. 2^31 - 1)"; }
        if (i && cuts[i] <= cuts[i - 1u]) { *at = i; return "not above the value in front of it (strictly ascending)"; }
    }
    return nullptr;
}
DCLC_FN Cuts make(const int32_t *cuts, u32 n) {      // (of a validated list)
    Cuts C;
    for (u32 i = 0; i < MAX_CUTS; i++) C.c[i] = i < n ? cuts[i] : 0;
    C.n = n;
    return C;
}

DCLC_FN u32 class_of(int32_t d, const Cuts &C) {
    u32 k = 0u;
    DBNC_UNROLL
    for (u32 j = 0; j < MAX_CUTS; j++) {
        if (j >= C.n) break;
        k += C.c[j] <= d ? 1u : 0u;
    }
    return k;
}

struct ClassView {
    Cuts cuts;
    DCLC_FN int32_t operator()(int32_t d) const { return d == dprc::PAD ? dprc::PAD : (int32_t)class_of(d, cuts); }
};

// The entries of word i of a region (drgc::Desc) that lie outside it become PAD.
DCLC_FN void mask_word(const drgc::Desc &d, u32 i, int32_t e[4]) {
    const u32 b0 = 4u * i - d.skip;      // as in drgc::add_word
    DBNC_UNROLL
    for (u32 j = 0; j < 4u; j++) e[j] = b0 + j < d.len ? e[j] : dprc::PAD;
}
// One lane's share of a masked word: cnt[t] += entries >= thr.c[t].  (The device counts the lanes' compare masks instead, see k_depth_regions_thr.)
DCLC_FN void count_word(const Cuts &thr, const int32_t e[4], u32 *cnt) {
    for (u32 t = 0; t < thr.n; t++)
        for (u32 j = 0; j < 4u; j++) cnt[t] += e[j] >= thr.c[t] ? 1u : 0u;
}

}  // namespace dclc
