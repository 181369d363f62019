// Genome entries on the device (cov_set_genomes): the contig-names genome scan (mosdepth_genome_coverage_with_contig_names,
// genome.rs:17-322) behind the pileup.  The per-contig accumulators (DevContig) are reduced over each genome's contigs, the depth
// histograms of a genome's contigs are merged, and calculate_coverage runs over genome entries through the same estimate_entry the
// contig kernels use (pileup_kernels.hip.h) — the float expressions exist once.
//
// The table genome -> contigs is a CSR (row[g] .. row[g + 1] into tids[], ascending tid inside a row).  Genome sizes are skewed (one
// "unbinned" genome of 10^5 contigs beside thousands of small ones), so rows are cut into SEGMENTS of at most GENOME_SEG contigs and the
// reduction and the histogram merge launch one wave per segment; a segment's partial results meet in the genome's accumulator through
// integer atomics (sums, min, max: any order gives the same bits).  The one f64 sum, sum_identity_nonsupp, is not associative: one wave
// per genome adds it contig by contig in ascending tid order, exactly as EntryAcc::add_contig does on the host.
#pragma once
#include "pileup_kernels.hip.h"

namespace covk {

constexpr u32 GENOME_SEG = 256;

// Per-genome accumulators (128 B): what EntryAcc holds after the add_contig of every seen contig, plus the unobserved lengths.
struct DevGenome {
    u64 reads;                       // sum of n_pass (genome.rs:173-174; n_nonsupp for separator entries): the entry's num_mapped_reads
    u64 sum_nm, sum_indel;
    u64 sum_d, sum_d2, cov_win, cov_full;
    u64 win_len, full_len, proc_win; // over the contigs with a considered record
    u64 unobs_win, unobs_full;       // over the others: with / without the contig_end_exclusion rule (estimators.rs:226-242)
    double id;                       // sum_identity_nonsupp, ascending tid order
    u64 hist_off;                    // its bins in the merged histogram
    u32 min_d, nh;                   // lowest window depth; bins = max over its windowed contigs of max_d + 1
    u32 n_seen, pad;
};
static_assert(sizeof(DevGenome) == 128, "DevGenome layout");

// mirrors cov_genome_stats (covermhip.h)
struct DevGenomeStats { u64 reads_in_genome, genome_len; u32 n_contigs_seen, any_nonzero; };

struct GenomeTable {
    const u32 *row;        // n_genomes + 1
    const u32 *tids;       // row[n_genomes] contigs
    const u32 *seg_genome; // n_seg
    const u32 *seg_start;  // n_seg: first entry of tids[]; the segment ends GENOME_SEG entries on, or with its genome's row
    u32 n_genomes, n_seg;
};

__global__ __launch_bounds__(256) void k_genome_init(DevGenome *__restrict__ G, u32 n_genomes) {
    const u32 g = blockIdx.x * 256u + threadIdx.x;
    if (g >= n_genomes) return;
    DevGenome z{};
    z.min_d = 0xffffffffu;
    G[g] = z;
}

// One wave per segment: the integer part of EntryAcc::add_contig over the segment's contigs, then one set of atomics per segment.
// `sep`: entries of the separator / single-genome scan (sep_kernels.hip.h) count a contig's reads as genome.rs:677-682 does (considered and
// not supplementary), the contig-names scan every considered record (genome.rs:173-174).
__global__ __launch_bounds__(256) void k_genome_reduce(const DevContig *__restrict__ ctg, const u32 *__restrict__ tlen, u64 excl, GenomeTable T,
                                                       DevGenome *__restrict__ G, u32 sep) {
    const u32 sg = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (sg >= T.n_seg) return;
    const u32 g = T.seg_genome[sg], lo = T.seg_start[sg], hi = min(lo + GENOME_SEG, T.row[g + 1]);
    u64 reads = 0, sum_nm = 0, sum_indel = 0, sum_d = 0, sum_d2 = 0, cov_win = 0, cov_full = 0, win_len = 0, full_len = 0, proc_win = 0, uw = 0, uf = 0;
    u32 min_d = 0xffffffffu, nh = 0, n_seen = 0;
    for (u32 i = lo + (u32)lane_id(); i < hi; i += 64u) {
        const u32 c = T.tids[i];
        const DevContig *C = &ctg[c];
        const u64 L = tlen[c];
        if (C->n_pass == 0) {                                  // an unobserved contig (genome.rs:252-262)
            uf += L; uw += L < 2 * excl ? L : L - 2 * excl;
            continue;
        }
        n_seen++;
        reads += sep ? C->n_nonsupp : C->n_pass; sum_nm += C->sum_nm; sum_indel += C->sum_indel;
        full_len += L; cov_full += C->cov_full;
        if (2 * excl < L) {                                    // estimators.rs:386-392, 436-445
            const u64 wl = L - 2 * excl;
            win_len += wl; sum_d += C->sum_d; sum_d2 += C->sum_d2; cov_win += C->cov_win; proc_win += C->proc_win;
            min_d = min(min_d, (C->proc_win < wl || C->min_d == 0xffffffffu) ? 0u : C->min_d);
            nh = max(nh, C->max_d + 1u);
        }
    }
    reads = wave_sum_u64(reads); sum_nm = wave_sum_u64(sum_nm); sum_indel = wave_sum_u64(sum_indel);
    sum_d = wave_sum_u64(sum_d); sum_d2 = wave_sum_u64(sum_d2); cov_win = wave_sum_u64(cov_win); cov_full = wave_sum_u64(cov_full);
    win_len = wave_sum_u64(win_len); full_len = wave_sum_u64(full_len); proc_win = wave_sum_u64(proc_win);
    uw = wave_sum_u64(uw); uf = wave_sum_u64(uf);
    min_d = wave_min_u32(min_d); nh = wave_max_u32(nh); n_seen = wave_sum_u32(n_seen);
    if (lane_id() != 0) return;
    DevGenome *A = &G[g];
    if (uw) atomicAdd(&A->unobs_win, uw);
    if (uf) atomicAdd(&A->unobs_full, uf);
    if (n_seen == 0) return;
    atomicAdd(&A->reads, reads); atomicAdd(&A->sum_nm, sum_nm); atomicAdd(&A->sum_indel, sum_indel);
    atomicAdd(&A->sum_d, sum_d); atomicAdd(&A->sum_d2, sum_d2); atomicAdd(&A->cov_win, cov_win); atomicAdd(&A->cov_full, cov_full);
    atomicAdd(&A->win_len, win_len); atomicAdd(&A->full_len, full_len); atomicAdd(&A->proc_win, proc_win);
    atomicMin(&A->min_d, min_d); atomicMax(&A->nh, nh); atomicAdd(&A->n_seen, n_seen);
}

// sum_identity_nonsupp of a genome: a strict chain of rounded f64 additions in ascending tid order (EntryAcc::add_contig, genome.rs:220-223).
// One wave per genome, as k_identity: 64 values per load (the next 64 are fetched while the chain of this batch runs), every lane replays
// the same 64 dependent adds from lane broadcasts.  A contig without a considered record holds +0.0, which leaves the sum's bits alone.
// `sep`: the separator scan adds the primary-read sum (genome.rs:724-727).
__global__ __launch_bounds__(64) void k_genome_identity(const DevContig *__restrict__ ctg, GenomeTable T, DevGenome *__restrict__ G, u32 sep) {
    const u32 g = blockIdx.x;
    if (g >= T.n_genomes) return;
    const u32 lo = T.row[g], hi = T.row[g + 1];
    double acc = 0.0;
    u32 i = lo + (u32)lane_id();
    double x = i < hi ? (sep ? ctg[T.tids[i]].id_primary : ctg[T.tids[i]].id_nonsupp) : 0.0;
    for (u32 b = lo; b < hi; b += 64u) {
        const double cur = x;
        i += 64u;
        x = i < hi ? (sep ? ctg[T.tids[i]].id_primary : ctg[T.tids[i]].id_nonsupp) : 0.0;
#pragma unroll 16
        for (int k = 0; k < 64; k++) acc += __shfl(cur, k);
    }
    if (lane_id() == 0) G[g].id = acc;
}

// Layout of the merged histogram: exclusive scan of the genomes' bin counts, in genome order (k_hist_sum / k_hist_off over genomes).
__global__ __launch_bounds__(1024) void k_genome_hist_sum(const DevGenome *__restrict__ G, u32 n_genomes, u64 *__restrict__ top) {
    __shared__ u64 wtot[16];
    const u32 g = blockIdx.x * 1024u + threadIdx.x;
    u64 total;
    (void)block_incl_scan<16>(g < n_genomes ? (u64)G[g].nh : 0ull, wtot, total);
    if (threadIdx.x == 0) top[blockIdx.x] = total;
}
__global__ __launch_bounds__(1024) void k_genome_hist_off(DevGenome *__restrict__ G, u32 n_genomes, const u64 *__restrict__ top, u64 *__restrict__ total_out,
                                                          u64 cap, DevGlobal *__restrict__ glob) {
    __shared__ u64 wtot[16];
    const u64 base = blocks_in_front<16>(top, wtot);
    const u32 g = blockIdx.x * 1024u + threadIdx.x;
    const u64 v = g < n_genomes ? (u64)G[g].nh : 0;
    u64 total;
    const u64 inc = block_incl_scan<16>(v, wtot, total);
    if (g < n_genomes) G[g].hist_off = base + inc - v;
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        *total_out = base + total;
        if (base + total > cap) glob->internal_error = 1u;      // (every genome bin is some contig's bin, so this holds; the finish fails if it ever does not)
    }
}
__global__ void k_zero_u64(u64 *__restrict__ p, const u64 *__restrict__ n_ptr, u64 cap) {
    const u64 n = min(*n_ptr, cap);
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) p[i] = 0ull;
}

// Merged bins of a genome = sums of its contigs' bins (EntryAcc::add_contig's histogram branch).  One wave per segment, a lane per bin (64
// bins at a time): the lane adds its bin over the segment's contigs in registers, then one atomic per (segment, bin) — the launch is
// sized by segments x bins, not by genomes.  The depth-0 positions of untouched tiles stay out, as in the arena: estimate_entry receives
// them as bin0_extra.
__global__ __launch_bounds__(256) void k_genome_hist_merge(const DevContig *__restrict__ ctg, const u32 *__restrict__ tlen, u64 excl,
                                                           const u32 *__restrict__ arena, GenomeTable T, const DevGenome *__restrict__ G,
                                                           u64 *__restrict__ ghist, u64 ghist_cap) {
    const u32 sg = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (sg >= T.n_seg) return;
    const u32 g = T.seg_genome[sg], lo = T.seg_start[sg], hi = min(lo + GENOME_SEG, T.row[g + 1]);
    const u32 nh = G[g].nh;
    const u64 goff = G[g].hist_off;
    if (nh == 0 || goff + nh > ghist_cap) return;
    for (u32 b = 0; b < nh; b += 64u) {
        const u32 d = b + (u32)lane_id();
        u64 acc = 0;
        for (u32 i = lo; i < hi; i++) {
            const u32 c = T.tids[i];
            const DevContig *C = &ctg[c];
            if (C->n_pass == 0 || !(2 * excl < (u64)tlen[c])) continue;
            if (d <= C->max_d) acc += arena[C->hist_off + d];
        }
        if (acc) atomicAdd(&ghist[goff + d], acc);
    }
}

// The order rule without the per-contig block on the host (cov_finish_genomes): over the contigs with a considered record, in tid order,
// first_rec must not lie before the largest last_rec in front (convert_results; contig.rs:129-132).  k_order_max leaves every block's
// largest last_rec + 1 (0: no seen contig) in ord[1 + block]; k_order_check scans and leaves the smallest offending first_rec in ord[0].
// (last_rec + 1 as a u64 would be needed at 2^32 - 1 records; the store holds at most 2^32 - 16)
__global__ __launch_bounds__(1024) void k_order_max(const DevContig *__restrict__ ctg, u32 n_targets, u64 *__restrict__ ord) {
    __shared__ u32 wmax[16];
    const u32 c = blockIdx.x * 1024u + threadIdx.x;
    u32 total;
    (void)block_incl_scan<16>((c < n_targets && ctg[c].n_pass != 0) ? ctg[c].last_rec + 1u : 0u, wmax, total, Max{});
    if (threadIdx.x == 0) ord[1 + blockIdx.x] = total;
    if (blockIdx.x == 0 && threadIdx.x == 0) ord[0] = ~0ull;
}
__global__ __launch_bounds__(1024) void k_order_check(const DevContig *__restrict__ ctg, u32 n_targets, u64 *__restrict__ ord) {
    __shared__ u32 wmax[16];
    const u32 base = blocks_in_front<16>(ord + 1, wmax, Max{});      // largest last_rec + 1 of the blocks in front
    const u32 c = blockIdx.x * 1024u + threadIdx.x;
    const bool seen = c < n_targets && ctg[c].n_pass != 0;
    const u32 v = seen ? ctg[c].last_rec + 1u : 0u;
    u32 total;
    const u32 inc = block_incl_scan<16>(v, wmax, total, Max{});
    const u32 prev = max(block_prev<16>(inc, wmax, 0u), base);      // exclusive prefix: the thread in front
    if (seen && prev != 0u && ctg[c].first_rec < prev - 1u) atomicMin(&ord[0], (u64)ctg[c].first_rec);
}

// calculate_coverage of every genome: entry = genome g (one wave per genome, or a lane per genome from 65 536 genomes on), its unobserved
// lengths the contigs of its row without a considered record.  Also leaves what the scan's control flow needs (cov_genome_stats).
template <bool LANES>
__device__ __forceinline__ void genome_estimate_body(const DevGenome *__restrict__ G, u32 n_genomes, const u64 *__restrict__ ghist, const EstParams &P,
                                                     float *__restrict__ out, DevGenomeStats *__restrict__ stats) {
    const u32 g_raw = LANES ? blockIdx.x * 256u + threadIdx.x : blockIdx.x * 4u + (threadIdx.x >> 6);
    if (!LANES && g_raw >= n_genomes) return;
    const bool in = g_raw < n_genomes;
    const u32 g = in ? g_raw : n_genomes - 1u;
    const DevGenome *A = &G[g];
    EstEntry E;
    E.win_len = A->win_len; E.win_sum_d = A->sum_d; E.win_sum_d2 = A->sum_d2; E.win_covered = A->cov_win; E.win_min_d = A->min_d;
    E.full_len = A->full_len; E.full_covered = A->cov_full; E.n_reads = A->reads; E.mismatches = A->sum_nm - A->sum_indel;
    E.nh = A->nh;
    E.bin0_extra = A->win_len - A->proc_win + A->unobs_win;      // counts[0] += unobserved (estimators.rs:596)
    E.unobs_win = A->unobs_win; E.unobs_full = A->unobs_full;
    E.identity = A->id;
    const bool nonzero = estimate_entry<LANES, u64>(E, ghist + A->hist_off, in, true, P, out + (size_t)g * P.n);
    if (LANES ? in : lane_id() == 0) {
        DevGenomeStats o;
        o.reads_in_genome = A->reads; o.genome_len = A->full_len + A->unobs_full; o.n_contigs_seen = A->n_seen; o.any_nonzero = nonzero ? 1u : 0u;
        stats[g] = o;
    }
}
__global__ __launch_bounds__(256) void k_genome_estimate(const DevGenome *__restrict__ G, u32 n_genomes, const u64 *__restrict__ ghist, EstParams P,
                                                         float *__restrict__ out, DevGenomeStats *__restrict__ stats) {
    genome_estimate_body<false>(G, n_genomes, ghist, P, out, stats);
}
__global__ __launch_bounds__(256) void k_genome_estimate_lanes(const DevGenome *__restrict__ G, u32 n_genomes, const u64 *__restrict__ ghist, EstParams P,
                                                               float *__restrict__ out, DevGenomeStats *__restrict__ stats) {
    genome_estimate_body<true>(G, n_genomes, ghist, P, out, stats);
}

}  // namespace covk
