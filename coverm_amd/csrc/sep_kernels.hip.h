// Separator / single-genome entries on the device (cov_set_genome_runs): the table entry -> contigs of mosdepth_genome_coverage
// (genome.rs:419-929) built per finish from two arrays — the genome id of every target (per header) and "the target has a considered
// record" (DevContig::n_pass, known behind k_prep) — by the rule of csrc/sep_entry_core.h, as prefix scans.  The table has the layout of
// GenomeTable (genome_kernels.hip.h), and the genome kernels then reduce, merge and evaluate over it as they do for cov_set_genomes.
//
// Device-wide scans in the two-launch pattern of k_genome_hist_sum / k_genome_hist_off: workgroups of sepc::SCAN_TILE = 1024 targets, a
// thread per target; the first launch leaves every workgroup's total, the second one has every workgroup fold the totals in front of it
// (behind it, for the scan from the right) and scan its own targets.
//   k_sep_obs_top    per workgroup: 1 + the last observed tid, and the first observed tid
//   k_sep_flags      prev1[] / next[] (running maximum, running minimum from the right), the start flag and the membership of every target
//                    (code[]), per workgroup the counts of starts and of members
//   k_sep_compact    inclusive scan of (starts, members): entry ids; members compacted in ascending tid order into tids[], their entry
//                    beside them; first_tid / gid of every entry; the two counts
//   k_sep_rows       row[]: where the entry changes along the compacted members
//   k_sep_seg_sum, k_sep_seg_write   rows cut into segments of GENOME_SEG members: an exclusive scan of ceil(len / GENOME_SEG) over the entries
// Every store is indexed by a scan value below the count the same scan ends in, and the host sizes every array for the largest count the
// header allows (members <= n_targets; entries <= runs of equal gid: two starts never share a run; segments <= entries + n_targets / GENOME_SEG).
#pragma once
#include "genome_kernels.hip.h"
#define SEPC_FN __host__ __device__ __forceinline__
#include "sep_entry_core.h"

namespace covk {

constexpr u32 SEP_TILE = sepc::SCAN_TILE;

struct SepEntry { u32 first_tid; int32_t gid; };      // of the entry's starting target q: blk[q], gid[q]

// counts[]: n_entries, n_members, n_seg
enum : u32 { SEP_N_ENTRIES = 0u, SEP_N_MEMBERS = 1u, SEP_N_SEG = 2u, SEP_N_COUNTS = 4u };

__global__ __launch_bounds__(1024) void k_sep_obs_top(const DevContig *__restrict__ ctg, u32 n_targets, u32 *__restrict__ top_last1, u32 *__restrict__ top_first) {
    __shared__ u32 wmax[16];
    const u32 t = blockIdx.x * SEP_TILE + threadIdx.x;
    const bool obs = t < n_targets && ctg[t].n_pass != 0;
    u32 last1, first_inv;
    (void)block_incl_scan<16>(obs ? t + 1u : 0u, wmax, last1, Max{});
    (void)block_incl_scan<16>(obs ? ~t : 0u, wmax, first_inv, Max{});      // (~t > 0 for every tid; 0 = none -> NONE)
    if (threadIdx.x == 0) { top_last1[blockIdx.x] = last1; top_first[blockIdx.x] = ~first_inv; }
}

__global__ __launch_bounds__(1024) void k_sep_flags(const DevContig *__restrict__ ctg, u32 n_targets, const int32_t *__restrict__ gid, const u32 *__restrict__ blk,
                                                    const u32 *__restrict__ top_last1, const u32 *__restrict__ top_first, uint8_t *__restrict__ code,
                                                    u64 *__restrict__ top_cnt) {
    __shared__ u32 wmax[16];
    __shared__ u64 wtot[16];
    __shared__ u32 s_prev1[SEP_TILE], s_next[SEP_TILE];
    const u32 b = blockIdx.x, nb = gridDim.x;
    const u32 base_prev1 = blocks_in_front<16>(top_last1, wmax, Max{});      // 1 + the nearest observed tid in front of this workgroup
    u32 mine = 0, base_next_inv, tot;
    for (u32 k = b + 1u + threadIdx.x; k < nb; k += SEP_TILE) mine = max(mine, ~top_first[k]);
    (void)block_incl_scan<16>(mine, wmax, base_next_inv, Max{});       // ~ the nearest observed tid behind it
    const u32 t = b * SEP_TILE + threadIdx.x;
    const bool obs = t < n_targets && ctg[t].n_pass != 0;
    const u32 prev1 = max(base_prev1, block_incl_scan<16>(obs ? t + 1u : 0u, wmax, tot, Max{}));
    // from the right: thread j scans target SEP_TILE - 1 - j of the workgroup
    const u32 jr = SEP_TILE - 1u - threadIdx.x, tr = b * SEP_TILE + jr;
    const bool obs_r = tr < n_targets && ctg[tr].n_pass != 0;
    const u32 next_inv = max(base_next_inv, block_incl_scan<16>(obs_r ? ~tr : 0u, wmax, tot, Max{}));
    s_prev1[threadIdx.x] = prev1; s_next[jr] = ~next_inv;
    __syncthreads();
    const u32 next = s_next[threadIdx.x];
    const u32 prev1_front = threadIdx.x ? s_prev1[threadIdx.x - 1u] : base_prev1;
    u32 start = 0, m = sepc::NOT_MEMBER;
    if (t < n_targets) {
        start = obs && sepc::starts_entry(gid, t, prev1_front) ? 1u : 0u;
        m = sepc::membership(gid, blk, t, obs, prev1, next);
        code[t] = (uint8_t)(start | (m << 1));
    }
    u64 total;
    (void)block_incl_scan<16>(((u64)start << 32) | (m != sepc::NOT_MEMBER ? 1ull : 0ull), wtot, total);
    if (threadIdx.x == 0) top_cnt[b] = total;
}

__global__ __launch_bounds__(1024) void k_sep_compact(u32 n_targets, const int32_t *__restrict__ gid, const u32 *__restrict__ blk, const uint8_t *__restrict__ code,
                                                      const u64 *__restrict__ top_cnt, u32 *__restrict__ tids, u32 *__restrict__ ent_of_pos,
                                                      SepEntry *__restrict__ ent, u32 ent_cap, u32 *__restrict__ counts, DevGlobal *__restrict__ glob) {
    __shared__ u64 wtot[16];
    const u64 base = blocks_in_front<16>(top_cnt, wtot);
    u64 total;
    const u32 t = blockIdx.x * SEP_TILE + threadIdx.x;
    const u32 c = t < n_targets ? code[t] : 0u, start = c & 1u, m = c >> 1;
    const u64 inc = base + block_incl_scan<16>(((u64)start << 32) | (m != sepc::NOT_MEMBER ? 1ull : 0ull), wtot, total);
    const u32 starts_incl = (u32)(inc >> 32);
    if (start && starts_incl - 1u < ent_cap) { SepEntry e; e.first_tid = blk[t]; e.gid = gid[t]; ent[starts_incl - 1u] = e; }
    if (m != sepc::NOT_MEMBER) {
        const u32 pos = (u32)inc - 1u;
        tids[pos] = t;
        ent_of_pos[pos] = m == sepc::MEMBER_OF_PREV ? starts_incl - 1u : starts_incl;
    }
    if (blockIdx.x == gridDim.x - 1u && threadIdx.x == 0) {
        const u32 n_entries = (u32)((base + total) >> 32);
        if (n_entries > ent_cap) glob->internal_error = 1u;      // (two starts never share a run of equal gid, so this holds; the finish fails if it ever does not)
        counts[SEP_N_ENTRIES] = min(n_entries, ent_cap); counts[SEP_N_MEMBERS] = (u32)(base + total);
    }
}

__global__ __launch_bounds__(256) void k_sep_rows(const u32 *__restrict__ counts, const u32 *__restrict__ ent_of_pos, u32 *__restrict__ row, u32 ent_cap) {
    const u32 i = blockIdx.x * 256u + threadIdx.x, n = counts[SEP_N_MEMBERS];
    if (i == 0 && n == 0) row[counts[SEP_N_ENTRIES]] = 0;      // (no member: no entry either)
    if (i >= n) return;
    const u32 e = ent_of_pos[i];
    if ((i == 0 || ent_of_pos[i - 1u] != e) && e < ent_cap) row[e] = i;
    if (i == n - 1u) row[counts[SEP_N_ENTRIES]] = n;
}

__device__ __forceinline__ u32 sep_segments_of(const u32 *__restrict__ row, u32 e) { return (row[e + 1u] - row[e] + GENOME_SEG - 1u) / GENOME_SEG; }

__global__ __launch_bounds__(1024) void k_sep_seg_sum(const u32 *__restrict__ counts, const u32 *__restrict__ row, u64 *__restrict__ top) {
    __shared__ u64 wtot[16];
    const u32 e = blockIdx.x * SEP_TILE + threadIdx.x;
    u64 total;
    (void)block_incl_scan<16>(e < counts[SEP_N_ENTRIES] ? (u64)sep_segments_of(row, e) : 0ull, wtot, total);
    if (threadIdx.x == 0) top[blockIdx.x] = total;
}
__global__ __launch_bounds__(1024) void k_sep_seg_write(u32 *__restrict__ counts, const u32 *__restrict__ row, const u64 *__restrict__ top, u32 *__restrict__ seg_genome,
                                                        u32 *__restrict__ seg_start, u32 seg_cap) {
    __shared__ u64 wtot[16];
    const u64 base = blocks_in_front<16>(top, wtot);
    u64 total;
    const u32 e = blockIdx.x * SEP_TILE + threadIdx.x;
    const u32 ns = e < counts[SEP_N_ENTRIES] ? sep_segments_of(row, e) : 0u;
    const u64 inc = base + block_incl_scan<16>((u64)ns, wtot, total);
    u32 sg = (u32)(inc - ns);
    for (u32 k = 0, i = ns ? row[e] : 0u; k < ns && sg < seg_cap; k++, sg++, i += GENOME_SEG) { seg_genome[sg] = e; seg_start[sg] = i; }
    if (blockIdx.x == gridDim.x - 1u && threadIdx.x == 0) counts[SEP_N_SEG] = (u32)min(base + total, (u64)seg_cap);
}

}  // namespace covk
