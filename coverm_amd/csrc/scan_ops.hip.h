// Prefix sums and their kin at the three levels every pass leans on, defined here and nowhere else:
//
//   wave       lane_id, the DPP inclusive scan / running maximum, a shuffle scan over any operator, the wave totals
//   workgroup  block_incl_scan<NW> over NW waves, block_prev<NW> (the value of the thread in front), blocks_in_front<NW> (the reduction of
//              the totals that the workgroups in front of this one left in an earlier launch)
//   device     k_scan_sums / k_scan_offsets / k_scan_apply: an exclusive u32 scan over any number of items in three launches
//
// Everything here is integer arithmetic, so the order of the additions is free.  The f64 identity sums (pileup_kernels.hip.h) are pinned to the
// reference's order and keep their own loops.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace covsc {

typedef unsigned long long u64;
typedef unsigned int u32;

// Operators of the generic scans.  T(0) must be their identity: sums, and maxima of unsigned values.
struct Plus { template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; } };
struct Max { template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a < b ? b : a; } };

// ---------------------------------------------------------------------------------------------- wave level
__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }

// Inclusive wave64 prefix sum with DPP lane moves (VALU latency, no LDS crossbar round trips):
// row_shr 1/2/4/8 inside each row of 16 lanes, then row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2-3.
__device__ __forceinline__ int wave_incl_scan(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);
    return v;
}
__device__ __forceinline__ u32 wave_incl_scan(u32 v) { return (u32)wave_incl_scan((int)v); }
// Inclusive wave64 running maximum (same DPP schedule as wave_incl_scan; lanes without a source keep INT_MIN).
__device__ __forceinline__ int wave_incl_max(int v) {
    const int NEG = (int)0x80000000;
    v = max(v, __builtin_amdgcn_update_dpp(NEG, v, 0x111, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(NEG, v, 0x112, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(NEG, v, 0x114, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(NEG, v, 0x118, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(NEG, v, 0x142, 0xa, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(NEG, v, 0x143, 0xc, 0xf, false));
    return v;
}
// Inclusive wave64 scan of any width over any operator, by shuffles (six LDS crossbar round trips per 32 bits).
template <typename T, typename Op>
__device__ __forceinline__ T wave_incl_scan(T v, Op op) {
    const int lane = lane_id();
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const T t = __shfl_up(v, o); if (lane >= o) v = op(v, t); }
    return v;
}
__device__ __forceinline__ u32 wave_incl_scan(u32 v, Plus) { return wave_incl_scan(v); }      // (a u32 sum takes the DPP schedule)
__device__ __forceinline__ u64 wave_incl_scan_u64(u64 v) { return wave_incl_scan(v, Plus{}); }

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ u32 wave_sum_u32(u32 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ u32 wave_min_u32(u32 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, (u32)__shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ u32 wave_max_u32(u32 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (u32)__shfl_xor(v, o));
    return v;
}

// Wave totals by DPP prefix sums (VALU only; the __shfl_xor versions above go through the LDS crossbar, twelve round trips for a u64).  Every lane
// returns the total.  wave_sum_u56: two 24-bit-apart halves, each summed in 32 bits — exact while the 64 values are below 2^50 (callers test that).
__device__ __forceinline__ u32 wave_sum_u32_dpp(u32 v) { return (u32)__builtin_amdgcn_readlane(wave_incl_scan((int)v), 63); }
__device__ __forceinline__ u64 wave_sum_u56(u64 v) {
    const u32 lo = (u32)v & 0xffffffu, hi = (u32)(v >> 24);
    return (u64)wave_sum_u32_dpp(lo) + ((u64)wave_sum_u32_dpp(hi) << 24);
}
__device__ __forceinline__ u32 wave_max_u32_dpp(u32 v) {      // (wave_incl_max compares as signed: flip the top bit)
    return (u32)__builtin_amdgcn_readlane(wave_incl_max((int)(v ^ 0x80000000u)), 63) ^ 0x80000000u;
}
__device__ __forceinline__ u32 wave_min_u32_dpp(u32 v) { return ~wave_max_u32_dpp(~v); }

// ---------------------------------------------------------------------------------------------- workgroup level
// NW is the number of waves of the caller's __launch_bounds__; every thread of the workgroup makes the call.
//
// The LDS contract, for all three functions: `lds` is NW words of T that the function owns for the length of the call.  No thread returns
// before every thread has read them, so the next call (these functions are called back to back on the same words), or any other use of the
// words by the caller, may follow without a barrier of the caller's.  A caller that wrote the words itself puts its own barrier in front.

// Inclusive scan over the workgroup's threads; `total` = the reduction over all of them.  An exclusive sum is the return value - v.
template <int NW, typename T, typename Op = Plus>
__device__ __forceinline__ T block_incl_scan(T v, T *lds, T &total, Op op = Op{}) {
    const int lane = lane_id(), w = (int)(threadIdx.x >> 6);
    const T inc = wave_incl_scan(v, op);
    if (lane == 63) lds[w] = inc;
    __syncthreads();
    T wbase = T(0), tot = T(0);
#pragma unroll
    for (int k = 0; k < NW; k++) { const T x = lds[k]; if (k < w) wbase = op(wbase, x); tot = op(tot, x); }
    __syncthreads();
    total = tot;
    return op(wbase, inc);
}
// x of the thread in front; thread 0 receives `first`.  (The exclusive form of a scan whose operator has no inverse, such as a maximum.)
template <int NW, typename T>
__device__ __forceinline__ T block_prev(T x, T *lds, T first) {
    const int lane = lane_id(), w = (int)(threadIdx.x >> 6);
    const T up = __shfl_up(x, 1);
    if (lane == 63) lds[w] = x;
    __syncthreads();
    const T prev = lane ? up : (w ? lds[w - 1] : first);
    __syncthreads();
    return prev;
}
// The second launch of a two-launch scan over workgroups: the reduction of top[0 .. blockIdx.x), the totals that the first launch left, returned
// to every thread (every workgroup reduces them itself: one value per workgroup in front).
template <int NW, typename S, typename T, typename Op = Plus>
__device__ __forceinline__ T blocks_in_front(const S *__restrict__ top, T *lds, Op op = Op{}) {
    T mine = T(0), base;
    for (u32 b = threadIdx.x; b < blockIdx.x; b += NW * 64u) mine = op(mine, (T)top[b]);
    (void)block_incl_scan<NW>(mine, lds, base, op);
    return base;
}

// ---------------------------------------------------------------------------------------------- device-wide exclusive u32 scan
// Three launches: per-block sums (4096 items per block), one workgroup scans the block sums, every block re-reads its items and
// hands (item, exclusive prefix) to the consumer.  F: value of item i; O: consumer.
constexpr u32 SCAN_ITEMS = 16, SCAN_BLOCK = 256 * SCAN_ITEMS;

template <typename F>
__global__ __launch_bounds__(256) void k_scan_sums(F f, u32 n, u32 *__restrict__ block_sums) {
    __shared__ u32 wsum[4];
    const u32 i0 = blockIdx.x * SCAN_BLOCK + threadIdx.x * SCAN_ITEMS;
    u32 s = 0;
    for (u32 k = 0; k < SCAN_ITEMS; k++) if (i0 + k < n) s += f(i0 + k);
    u32 total;
    (void)block_incl_scan<4>(s, wsum, total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}
// block_sums[0 .. nb) -> exclusive prefixes in place, grand total at block_sums[nb]  (64-bit total at total64)
__global__ __launch_bounds__(1024) void k_scan_offsets(u32 *__restrict__ block_sums, u32 nb, u64 *__restrict__ total64) {
    __shared__ u64 part[1024];
    const u32 t = threadIdx.x, per = (nb + 1023u) / 1024u, k0 = t * per, k1 = min(nb, k0 + per);
    u64 s = 0;
    for (u32 k = k0; k < k1; k++) s += block_sums[k];
    part[t] = s;
    __syncthreads();
    if (t == 0) { u64 a = 0; for (u32 i = 0; i < 1024; i++) { const u64 x = part[i]; part[i] = a; a += x; } *total64 = a; }
    __syncthreads();
    u64 a = part[t];
    for (u32 k = k0; k < k1; k++) { const u32 x = block_sums[k]; block_sums[k] = (u32)a; a += x; }
    if (t == 0) block_sums[nb] = (u32)*total64;
}
template <typename F, typename O>
__global__ __launch_bounds__(256) void k_scan_apply(F f, O out, u32 n, const u32 *__restrict__ block_offs) {
    __shared__ u32 wsum[4];
    const u32 i0 = blockIdx.x * SCAN_BLOCK + threadIdx.x * SCAN_ITEMS;
    u32 v[SCAN_ITEMS], s = 0;
    for (u32 k = 0; k < SCAN_ITEMS; k++) { v[k] = i0 + k < n ? f(i0 + k) : 0u; s += v[k]; }
    u32 total;
    u32 p = block_offs[blockIdx.x] + block_incl_scan<4>(s, wsum, total) - s;
    for (u32 k = 0; k < SCAN_ITEMS; k++) { if (i0 + k < n) out(i0 + k, p); p += v[k]; }
}

}  // namespace covsc
