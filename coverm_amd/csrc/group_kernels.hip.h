// cov_group_records: the records of every reference made contiguous on the device — a stable LSD radix sort of record indices by
// key = tid (n_targets for records without a reference, which come last), then one gather of the store.  A mapper writes its records
// in read order; the pipeline only needs the records of one reference to be contiguous (it walks position-unsorted contigs already),
// so this replaces `samtools sort` for a sample that fits the record store.
//
//   k_group_check     does a key ever decrease?  When not, nothing else runs: a grouped file pays one read of the tid column.
//   per pass (digit of 8 bits, grpk::n_passes(n_targets) of them):
//     k_group_hist    digit histogram of every workgroup's tile of 4096 items, stored digit-major
//     covsc::k_scan_* ONE exclusive scan over [digit][workgroup] (the device-wide scan of scan_ops.hip.h): base[d][wg]
//     k_group_scatter item -> base + rank inside the tile.  The rank is counted, never raced for: per round of 256 items the lanes of a wave
//                     find their peers (same digit) with eight ballots, the lowest peer posts the wave's count in LDS, the digit's thread turns
//                     the four counts into four bases (group_rank_core.h, shared with the CPU emulation of tests/c/group_rank_host.cpp).
//                     Keys travel with the indices (the first pass reads tid itself and needs no index array, the last writes no keys).
//   k_group_moved     records whose index changed
//   gather            covp::SelCigarLen scan + covp::SelGather (the pair filter's), k_group_gather_mates for the mate columns
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define GRPK_FN __host__ __device__ __forceinline__
#include "group_rank_core.h"

namespace covg {

typedef unsigned long long u64;
typedef unsigned int u32;

// out[0] = 1 when some key is lower than its predecessor's (every finder stores the same value: no order to decide)
__global__ __launch_bounds__(256) void k_group_check(const int32_t *__restrict__ tid, u32 n, u32 n_targets, u32 *__restrict__ out) {
    bool bad = false;
    for (u64 i = (u64)blockIdx.x * 256u + threadIdx.x + 1u; i < n; i += (u64)gridDim.x * 256u)
        bad |= grpk::key_of(tid[i], n_targets) < grpk::key_of(tid[i - 1], n_targets);
    if (bad) out[0] = 1u;
}

template <bool FIRST>
__device__ __forceinline__ u32 load_key(const int32_t *__restrict__ tid, const u32 *__restrict__ key_in, u64 i, u32 n_targets) {
    return FIRST ? grpk::key_of(tid[i], n_targets) : key_in[i];
}

template <bool FIRST>
__global__ __launch_bounds__(256) void k_group_hist(const int32_t *__restrict__ tid, const u32 *__restrict__ key_in, u32 n, u32 n_targets, u32 pass, u32 *__restrict__ hist, u32 n_wg) {
    __shared__ u32 h[grpk::RADIX];
    const u32 t = threadIdx.x;
    h[t] = 0u;
    __syncthreads();
    const u64 i0 = (u64)blockIdx.x * grpk::TILE + t;
    for (u32 r = 0; r < grpk::ITEMS; r++) {
        const u64 i = i0 + r * grpk::WG;
        if (i < n) atomicAdd(&h[grpk::digit_of(load_key<FIRST>(tid, key_in, i, n_targets), pass)], 1u);      // a count: the same whatever the order
    }
    __syncthreads();
    hist[grpk::hist_index(t, blockIdx.x, n_wg)] = h[t];
}

struct HistVal { const u32 *h; __device__ u32 operator()(u32 i) const { return h[i]; } };
struct HistPut { u32 *b; __device__ void operator()(u32 i, u32 p) const { b[i] = p; } };

// idx_in == nullptr on the first pass (the index of item i is i); key_out == nullptr on the last.
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(256) void k_group_scatter(const int32_t *__restrict__ tid, const u32 *__restrict__ key_in, const u32 *__restrict__ idx_in, u32 *__restrict__ key_out,
                                                       u32 *__restrict__ idx_out, u32 n, u32 n_targets, u32 pass, const u32 *__restrict__ base, u32 n_wg) {
    __shared__ u32 running[grpk::RADIX];
    __shared__ u32 wcnt[2][grpk::WAVES][grpk::RADIX];      // two sets in turn: the digit's thread clears the idle one while it serves the other
    const u32 t = threadIdx.x, lane = t & 63u, w = t >> 6;
    running[t] = base[grpk::hist_index(t, blockIdx.x, n_wg)];
    for (u32 k = 0; k < grpk::WAVES; k++) { wcnt[0][k][t] = 0u; wcnt[1][k][t] = 0u; }
    __syncthreads();
    const u64 i0 = (u64)blockIdx.x * grpk::TILE + t;
    for (u32 r = 0; r < grpk::ITEMS; r++) {
        const u32 set = r & 1u;
        const u64 i = i0 + r * grpk::WG;
        const bool valid = i < n;
        const u32 key = valid ? load_key<FIRST>(tid, key_in, i, n_targets) : 0u;
        const u32 d = grpk::digit_of(key, pass);
        u64 peers = __ballot(valid);
        for (u32 b = 0; b < grpk::RADIX_BITS; b++) peers = grpk::peers_step(peers, d, b, __ballot(valid && ((d >> b) & 1u)));
        const u32 rank = grpk::rank_among(peers, lane);
        if (valid && grpk::is_leader(peers, lane)) wcnt[set][w][d] = grpk::popc(peers);
        __syncthreads();
        {   // digit t: the waves' counts become the waves' bases
            u32 cnt[grpk::WAVES], out[grpk::WAVES];
            for (u32 k = 0; k < grpk::WAVES; k++) cnt[k] = wcnt[set][k][t];
            running[t] = grpk::wave_bases(running[t], cnt, out);
            for (u32 k = 0; k < grpk::WAVES; k++) { wcnt[set][k][t] = out[k]; wcnt[set ^ 1u][k][t] = 0u; }
        }
        __syncthreads();
        if (valid) {
            const u32 p = wcnt[set][w][d] + rank;
            if (p < n) {      // (always: the bases come from the histogram of these very digits)
                idx_out[p] = FIRST ? (u32)i : idx_in[i];
                if (!LAST) key_out[p] = key;
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_group_moved(const u32 *__restrict__ order, u32 n, u64 *__restrict__ out) {
    u32 c = 0;
    for (u64 i = (u64)blockIdx.x * 256u + threadIdx.x; i < n; i += (u64)gridDim.x * 256u) c += order[i] != (u32)i ? 1u : 0u;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, (u64)c);      // a sum
}

__global__ __launch_bounds__(256) void k_group_gather_mates(const u32 *__restrict__ order, u32 n, const int32_t *__restrict__ mtid, const u64 *__restrict__ qh1, const u32 *__restrict__ qh2,
                                                            int32_t *__restrict__ o_mtid, u64 *__restrict__ o_qh1, u32 *__restrict__ o_qh2) {
    const u64 p = (u64)blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    const u32 j = order[p];
    o_mtid[p] = mtid[j]; o_qh1[p] = qh1[j]; o_qh2[p] = qh2[j];
}

}  // namespace covg
