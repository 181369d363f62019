// Admission of one window of ingested records to the bounded record store (admit_window in covermhip.hip, for the BGZF ingest and the SAM
// text ingest alike): does the store spill first, does the window pass the hard limit, how large is the store made for the first of several
// windows.  Arithmetic only, no HIP: tests/c/store_plan_host.cpp runs it on the CPU against the formulas the two ingests carried.
#pragma once

namespace stplan {
typedef unsigned long long u64;
constexpr u64 HARD_LIMIT = 0xfffffff0ull;      // 2^32 - 16 records, and as many CIGAR words: indices are 32 bits wide on the device
constexpr u64 SLACK = 1024;
inline bool past_limit(u64 have, u64 add) { return have + add >= HARD_LIMIT; }

// The window would take the store past a cap: what has been extracted is sealed and spilled first, the window follows the contig in flight.
// Not with an empty store (nothing could leave), not with mate columns (a spill does not move them), not after a failure (no extraction).
inline bool spill_first(bool store_empty, bool mates_wanted, bool failure_pending, bool over_record_cap, bool over_cigar_cap) {
    return !store_empty && !mates_wanted && !failure_pending && (over_record_cap || over_cigar_cap);
}

// First of several windows: the store is sized for the whole file at once, `scale` times what this window holds.  (A store sized per window
// grows with every later one — allocate, copy, drain the device, free: 0.8 s of stalls at 100 M reads, profiles/r04_timeline_store_regrowth.txt.)
// have = elements in front of the window, add = the window's own, spare = 1 for the CIGAR column's spare word.  Never less than the window
// needs, and beyond that never past the cap: what would lie behind it is spilled before it is written.
inline u64 first_window_size(u64 have, u64 add, u64 spare, double scale, u64 cap) {
    const u64 need = have + add + spare, whole = have + (u64)((double)add * scale) + SLACK;
    const u64 ceiling = cap + SLACK < HARD_LIMIT ? cap + SLACK : HARD_LIMIT;
    const u64 bounded = whole < ceiling ? whole : ceiling;
    return need > bounded ? need : bounded;
}
}  // namespace stplan
