// Separator / single-genome entries (mosdepth_genome_coverage, genome.rs:419-929; covh_genome_coverage_separator): which contigs form an
// entry and which contigs without a read count as its unobserved lengths — the rule written once, run two ways (the kernels of
// csrc/sep_kernels.hip.h; serially on the CPU in entries_cpu below, which tests/c/sep_entry_host.cpp checks against a walk that mirrors
// fill_backwards / fill_backwards_to_last / fill_forwards, and which host_coverage.cpp aggregates over).
//
// Per target t in header order: gid[t] = dense id of the name's prefix before the separator (all 0 in single-genome mode), obs[t] = the
// target has a considered record (n_pass > 0).  blk[t] = first tid of the maximal run of equal gid containing t (header only).
//   prev1[t] = 1 + the nearest observed tid <= t, 0 = none         (a running maximum of obs ? t + 1 : 0)
//   next[t]  = the nearest observed tid >= t, NONE = none          (a running minimum from the right)
// An observed q STARTS an entry iff no observed target lies in front of it or the nearest one, p, has gid[p] != gid[q].  Entries are
// numbered in tid order of their starting targets: with starts_incl[t] = starts among the targets 0 .. t,
//   an observed t is a member of entry starts_incl[t] - 1;
//   an unobserved t behind an observed p of its own block (p >= blk[t]) is a member of p's entry, starts_incl[t] - 1: the forward
//     extension of fill_backwards_to_last / fill_forwards, stopped by the first foreign name;
//   else an unobserved t in front of an observed q of its own block is a member of q's entry iff q starts one (fill_backwards runs at an
//     entry's start only), and that entry is starts_incl[t] (no start lies between t and q);
//   else t belongs to no entry (A(obs) B A A(obs): the A behind B).
// The entry's first_tid is blk[q] of its starting target q, its members are ascending tids, and entries ascend in tid: the table
// entry -> members is one stable compaction of the member targets.
#pragma once
#include <stdint.h>

#ifndef SEPC_FN
#define SEPC_FN inline
#endif

namespace sepc {

typedef unsigned int u32;

constexpr u32 NONE = 0xffffffffu;
constexpr u32 SCAN_TILE = 1024u;      // targets per workgroup of the device-wide scans (sep_kernels.hip.h): one thread each

enum : u32 { NOT_MEMBER = 0u, MEMBER_OF_PREV = 1u, MEMBER_OF_NEXT = 2u };

// `prev1_front` = prev1 of the target in front of q (0 for q = 0)
SEPC_FN bool starts_entry(const int32_t *gid, u32 q, u32 prev1_front) { return prev1_front == 0u || gid[prev1_front - 1u] != gid[q]; }

// Which entry target t counts for: MEMBER_OF_PREV -> entry starts_incl[t] - 1, MEMBER_OF_NEXT -> entry starts_incl[t].
SEPC_FN u32 membership(const int32_t *gid, const u32 *blk, u32 t, bool obs, u32 prev1, u32 next) {
    if (obs) return MEMBER_OF_PREV;
    if (prev1 != 0u && prev1 - 1u >= blk[t]) return MEMBER_OF_PREV;
    // (t is unobserved, so the nearest observed target in front of `next` is the one in front of t)
    if (next != NONE && blk[next] == blk[t] && starts_entry(gid, next, prev1)) return MEMBER_OF_NEXT;
    return NOT_MEMBER;
}

SEPC_FN void blocks_of(const int32_t *gid, u32 n, u32 *blk) {
    for (u32 t = 0; t < n; t++) blk[t] = (t != 0u && gid[t] == gid[t - 1u]) ? blk[t - 1u] : t;
}

// The table on the CPU, scan by scan as the kernels build it.  row[] takes n_entries + 1 values (at most n + 1), tids[] and the entry
// arrays at most n.  Returns the number of entries.
SEPC_FN u32 entries_cpu(const int32_t *gid, const uint8_t *obs, u32 n, u32 *blk, u32 *prev1, u32 *next, u32 *row, u32 *tids, u32 *first_tid,
                        int32_t *entry_gid) {
    blocks_of(gid, n, blk);
    for (u32 t = 0, p = 0u; t < n; t++) { if (obs[t]) p = t + 1u; prev1[t] = p; }
    for (u32 t = n, q = NONE; t-- > 0u;) { if (obs[t]) q = t; next[t] = q; }
    u32 starts = 0, members = 0, last_entry = NONE;
    for (u32 t = 0; t < n; t++) {
        if (obs[t] && starts_entry(gid, t, t ? prev1[t - 1u] : 0u)) { first_tid[starts] = blk[t]; entry_gid[starts] = gid[t]; starts++; }
        const u32 m = membership(gid, blk, t, obs[t] != 0, prev1[t], next[t]);
        if (m == NOT_MEMBER) continue;
        const u32 e = m == MEMBER_OF_PREV ? starts - 1u : starts;
        if (e != last_entry) { row[e] = members; last_entry = e; }
        tids[members++] = t;
    }
    row[starts] = members;
    return starts;
}

}  // namespace sepc
