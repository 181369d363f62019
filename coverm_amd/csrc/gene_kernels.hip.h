// cov_interval_reads_compute: the per-gene read aggregates of --gff (genes.rs:206-304, 493-524) from the session's record store — what
// covh_gene_coverage's record pass computes on the host from the records copied back, here without the records leaving the device.
// The arithmetic that needs no wave is csrc/gene_reads_core.h (shared with the CPU emulation of tests/c/gene_reads_host.cpp).
//
//   k_gene_classify   a record per lane: skip | take | NM error, the primary bit, mism, the read's identity; an NM error posts its
//                     verdict key; per tile of 1024 records the counts of taken / primary records and the sum of mism
//   k_gene_offsets    ONE exclusive scan over the tiles' sums (a single workgroup; the totals close the prefix arrays)
//   k_gene_scatter    the taken records compacted in file order: tid, pos, record index, identity, and the exclusive prefix sums of the
//                     primary bit and of mism (wrapping: only differences are used)
//   k_gene_order      a taken record against the one in front of it: tid decreases / tid outside the header (verdict keys), and
//                     "a start decreases inside a contig" (then lower_bound is not defined and the caller takes the host path)
//   k_gene_bounds     a gene per thread: the contig's slice of the taken records, lo / hi = lower_bound of the gene's ends over the
//                     slice's starts, n_reads and mismatches as differences of the prefixes
//   k_gene_ckpt       (identity) a wave per contig with genes: P, the serial f64 running sum of the identities from the slice's first
//                     record (genes.rs:500), kept at every 1024th record.  f64 addition is not associative: the sum is replayed in order,
//                     64 records per step by id_block_add (pileup_kernels.hip.h, the body k_id_combine runs)
//   k_gene_ident      (identity) a wave per gene: P[lo] and P[hi], each replayed from the checkpoint at or below it (at most 16 blocks;
//                     lanes at or beyond the boundary add +0.0, which leaves S as it is); sum_identity = P[hi] - P[lo]
#pragma once
#include "pileup_kernels.hip.h"

#define GNRC_FN __host__ __device__ __forceinline__
#include "gene_reads_core.h"

namespace covgn {

using covk::u32;
using covk::u64;

constexpr u32 TILE = 1024u, WG = 256u, ITEMS = TILE / WG;
enum : u32 { G_VERDICT = 0u, G_UNSORTED = 1u, G_TAKEN = 2u, G_MAPPED = 3u, G_COUNT = 4u };      // the words the host reads back

struct Work {
    uint8_t *code;              // per record: state | primary << 2
    u32 *mism;                  // per record: NM.saturating_sub(indels) (NM is 32 bits wide)
    double *ident;              // per record (want_identity), else nullptr
    u64 *b_cnt, *b_mism;        // per tile: taken | primary << 32, sum of mism; exclusive after k_gene_offsets
    int32_t *t_tid, *t_pos;     // the taken records in file order ...
    u32 *t_rec, *pprim;         // ... their record index; exclusive prefix of the primary bit (T + 1 entries, mod 2^32: a difference is below 2^32)
    u64 *pmism;                 // exclusive prefix of mism (T + 1 entries)
    double *t_ident;            // (want_identity)
    u64 *glob;                  // G_*
};

struct Bounds { u32 cs, lo, hi, k; };      // a gene's slice start, its two boundaries, its contig's number among the contigs with genes
struct Out { u64 n_reads, mismatches; double sum_identity; u64 contig_taken; };

__device__ __forceinline__ u64 wave_min_u64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const u64 t = __shfl_xor(v, o); v = t < v ? t : v; }
    return v;
}
__device__ __forceinline__ void post_verdict(u64 *glob, u64 key) {      // the whole wave calls it
    if (__ballot(key != gnrc::NO_VERDICT) == 0ull) return;
    const u64 m = wave_min_u64(key);
    if (covk::lane_id() == 0) atomicMin((unsigned long long *)&glob[G_VERDICT], (unsigned long long)m);
}
using covsc::block_incl_scan;      // (the sums below wrap; an exclusive prefix is the inclusive one less the thread's own value)

__global__ __launch_bounds__(256) void k_gene_classify(const covk::Records r, const gnrc::Filter f, Work w) {
    __shared__ u64 s_cnt[4], s_mism[4];
    const u64 base = (u64)blockIdx.x * TILE;
    u64 cnt = 0, msum = 0;
    for (u32 k = 0; k < ITEMS; k++) {
        const u64 i = base + (u64)k * WG + threadIdx.x;
        u64 key = gnrc::NO_VERDICT;
        if (i < r.n) {
            u64 aligned = 0, indels = 0;
            const u32 c0 = r.cigar_off[i], c1 = r.cigar_off[i + 1];
            for (u32 c = c0; c < c1; c++) gnrc::cigar_add(r.cigar[c], aligned, indels);
            const gnrc::Class c = gnrc::classify(f, r.flag[i], r.mapq[i], r.nm_kind[i], r.nm[i], r.l_seq[i], aligned, indels);
            w.code[i] = (uint8_t)(c.state | (c.primary << 2));
            w.mism[i] = (u32)c.mism;
            if (w.ident) w.ident[i] = c.ident;
            if (c.state == gnrc::TAKE) { cnt += 1ull + ((u64)c.primary << 32); msum += c.mism; }
            else if (c.state != gnrc::SKIP) key = gnrc::verdict_key(i, c.state == gnrc::NM_MISSING ? gnrc::RULE_NM_MISSING : gnrc::RULE_NM_BADTYPE);
        }
        post_verdict(w.glob, key);
    }
    cnt = covk::wave_sum_u64(cnt); msum = covk::wave_sum_u64(msum);
    if ((threadIdx.x & 63u) == 0u) { s_cnt[threadIdx.x >> 6] = cnt; s_mism[threadIdx.x >> 6] = msum; }
    __syncthreads();
    if (threadIdx.x == 0) { w.b_cnt[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3]; w.b_mism[blockIdx.x] = s_mism[0] + s_mism[1] + s_mism[2] + s_mism[3]; }
}

// One workgroup: b_cnt / b_mism become exclusive prefixes over the nb tiles (the two halves of b_cnt scanned apart and packed again).
__global__ __launch_bounds__(1024) void k_gene_offsets(Work w, u32 nb) {
    __shared__ u64 lds[16];
    u64 c_taken = 0, c_prim = 0, c_mism = 0;
    for (u32 b0 = 0; b0 < nb; b0 += 1024u) {
        const u32 b = b0 + threadIdx.x;
        const u64 cnt = b < nb ? w.b_cnt[b] : 0ull, ms = b < nb ? w.b_mism[b] : 0ull;
        const u64 taken = cnt & 0xffffffffull, prim = cnt >> 32;
        u64 t_tot, p_tot, m_tot;
        const u64 t_ex = block_incl_scan<16>(taken, lds, t_tot) - taken;
        const u64 p_ex = block_incl_scan<16>(prim, lds, p_tot) - prim;
        const u64 m_ex = block_incl_scan<16>(ms, lds, m_tot) - ms;
        if (b < nb) { w.b_cnt[b] = ((c_taken + t_ex) & 0xffffffffull) | ((c_prim + p_ex) << 32); w.b_mism[b] = c_mism + m_ex; }
        c_taken += t_tot; c_prim += p_tot; c_mism += m_tot;
    }
    if (threadIdx.x == 0) {
        w.glob[G_TAKEN] = c_taken; w.glob[G_MAPPED] = c_prim;
        w.pprim[c_taken] = (u32)c_prim; w.pmism[c_taken] = c_mism;      // the closing entries of the two prefixes
    }
}

// Thread t of a tile holds its records 4 t .. 4 t + 3: thread order, then item order, is file order.
__global__ __launch_bounds__(256) void k_gene_scatter(const covk::Records r, Work w) {
    __shared__ u64 lds[4];
    const u64 base = (u64)blockIdx.x * TILE + (u64)threadIdx.x * ITEMS;
    u32 code[ITEMS], ms[ITEMS];
    u64 cnt = 0, msum = 0;
#pragma unroll
    for (u32 k = 0; k < ITEMS; k++) {
        const u64 i = base + k;
        code[k] = i < r.n ? w.code[i] : 0u;
        const bool take = (code[k] & 3u) == gnrc::TAKE;
        ms[k] = take ? w.mism[i] : 0u;
        if (take) { cnt += 1ull + ((u64)(code[k] >> 2) << 32); msum += ms[k]; }
    }
    u64 tot;
    const u64 c_ex = block_incl_scan<4>(cnt, lds, tot) - cnt, m_ex = block_incl_scan<4>(msum, lds, tot) - msum;      // (a tile's counts stay below 2^32: no carry between the halves)
    const u64 b_cnt = w.b_cnt[blockIdx.x];
    u32 j = (u32)b_cnt + (u32)c_ex, p = (u32)(b_cnt >> 32) + (u32)(c_ex >> 32);
    u64 m = w.b_mism[blockIdx.x] + m_ex;
#pragma unroll
    for (u32 k = 0; k < ITEMS; k++) {
        if ((code[k] & 3u) != gnrc::TAKE) continue;
        const u64 i = base + k;
        w.t_tid[j] = r.tid[i]; w.t_pos[j] = r.pos[i]; w.t_rec[j] = (u32)i; w.pprim[j] = p; w.pmism[j] = m;
        if (w.t_ident) w.t_ident[j] = w.ident[i];
        j++; p += code[k] >> 2; m += ms[k];
    }
}

__global__ __launch_bounds__(256) void k_gene_order(Work w, u32 n_targets) {
    const u64 T = w.glob[G_TAKEN];
    const u64 stride = (u64)gridDim.x * 256u;
    const u64 rounds = (T + stride - 1) / stride;      // every lane of a wave makes the same number of rounds: post_verdict is a wave's call
    bool dec = false;
    for (u64 q = 0; q < rounds; q++) {
        const u64 j = q * stride + (u64)blockIdx.x * 256u + threadIdx.x;
        u64 key = gnrc::NO_VERDICT;
        if (j < T) {
            const int32_t tid = w.t_tid[j], prev = j ? w.t_tid[j - 1] : -2;
            key = gnrc::order_verdict(w.t_rec[j], tid, prev, n_targets);
            dec |= j != 0 && tid == prev && gnrc::start_of(w.t_pos[j]) < gnrc::start_of(w.t_pos[j - 1]);
        }
        post_verdict(w.glob, key);
    }
    if (dec) w.glob[G_UNSORTED] = 1ull;      // every finder stores the same value
}

// iv[g].pad = the number of the gene's contig among the contigs with genes (the host numbers them)
__global__ __launch_bounds__(256) void k_gene_bounds(const Work w, const gnrc::Interval *__restrict__ iv, u64 n, Out *__restrict__ out, Bounds *__restrict__ bounds) {
    const u32 T = (u32)w.glob[G_TAKEN];
    for (u64 g = (u64)blockIdx.x * 256u + threadIdx.x; g < n; g += (u64)gridDim.x * 256u) {
        const gnrc::Interval v = iv[g];
        const u32 cs = gnrc::lower_bound_tid(w.t_tid, 0u, T, (long long)v.tid), ce = gnrc::lower_bound_tid(w.t_tid, cs, T, (long long)v.tid + 1);
        const u32 lo = gnrc::lower_bound_start(w.t_pos, cs, ce, v.start), hi = gnrc::lower_bound_start(w.t_pos, cs, ce, v.end);
        Out o;
        o.n_reads = (u64)(u32)(w.pprim[hi] - w.pprim[lo]); o.mismatches = w.pmism[hi] - w.pmism[lo]; o.sum_identity = 0.0; o.contig_taken = ce - cs;
        out[g] = o;
        Bounds b; b.cs = cs; b.lo = lo; b.hi = hi; b.k = v.pad;
        bounds[g] = b;
    }
}

// gene_tids[k] = the k-th contig with genes, ascending
__global__ __launch_bounds__(64) void k_gene_ckpt(const Work w, const u32 *__restrict__ gene_tids, u32 n_contigs, double *__restrict__ ck) {
    const u32 k = blockIdx.x;
    if (k >= n_contigs) return;
    const int lane = covk::lane_id();
    const u32 T = (u32)w.glob[G_TAKEN];
    const long long tid = (long long)gene_tids[k];
    const u32 cs = gnrc::lower_bound_tid(w.t_tid, 0u, T, tid), ce = gnrc::lower_bound_tid(w.t_tid, cs, T, tid + 1);
    double *slot = ck + gnrc::ck_base(cs, k);
    double S = 0.0;
    double x = (u64)cs + (u32)lane < ce ? w.t_ident[(u64)cs + (u32)lane] : 0.0;
    for (u32 b = cs; b < ce; b += 64u) {
        if (((b - cs) & (gnrc::CK - 1u)) == 0u && lane == 0) slot[(b - cs) / gnrc::CK] = S;
        const double cur = x;
        const u64 nx = (u64)b + 64u + (u32)lane;
        x = nx < ce ? w.t_ident[nx] : 0.0;      // the next block's values are in flight during this one
        covk::id_block_add(S, cur, lane);
    }
    if (((ce - cs) & (gnrc::CK - 1u)) == 0u && lane == 0) slot[(ce - cs) / gnrc::CK] = S;
}

__global__ __launch_bounds__(64) void k_gene_ident(const Work w, const Bounds *__restrict__ bounds, u64 n, const double *__restrict__ ck, Out *__restrict__ out) {
    const u64 g = blockIdx.x;
    if (g >= n) return;
    const int lane = covk::lane_id();
    const Bounds b = bounds[g];
    if (b.lo == b.hi) return;      // P - P
    const double *slot = ck + gnrc::ck_base(b.cs, b.k);
    double P[2];
#pragma unroll
    for (int e = 0; e < 2; e++) {
        const u32 at = e ? b.hi : b.lo, m = (at - b.cs) / gnrc::CK;
        double S = slot[m];
        for (u32 b0 = b.cs + m * gnrc::CK; b0 < at; b0 += 64u) {
            const u64 j = (u64)b0 + (u32)lane;
            covk::id_block_add(S, j < at ? w.t_ident[j] : 0.0, lane);
        }
        P[e] = S;
    }
    if (lane == 0) out[g].sum_identity = P[1] - P[0];
}

}  // namespace covgn
