// cov_depth_bins_*: sum, min, max and covered bases of the per-base depth over fixed windows, reduced on the device from the chunk's arena
// (the arena, start mask and rank of cov_depth_runs_*, depth_kernels.hip.h).  The arithmetic is csrc/depth_bins_core.h, shared with the CPU
// emulation of tests/c/depth_bins_host.cpp.
//
//   k_bins_init    a bin per thread: (0, INT32_MAX, 0, 0, 0), what the atomics of shared bins merge into
//   k_depth_bins   a wave owns a contiguous stretch of dbnc::STRETCH_WORDS arena words and walks it in dbnc::WAVE_STEPS steps of 64 words:
//                  lane i of step j loads word base + 64 j + i with one 16-byte load (the wave reads a contiguous KiB per instruction, the
//                  next step's word is in flight while this one is reduced) and forms the word's partials (one to four bins, all of one
//                  target).  The global bin id never decreases along the arena, so equal ids are contiguous in lane order: a segmented
//                  scan over the lanes (six shuffle rounds) reduces the partials that share a bin, and the bin still open at lane 63 is
//                  carried in registers into the next step.  A lane whose word touches several bins feeds the scan its LAST partial; its
//                  first one closes in the lane (merged with what the lanes in front hold of that bin), the ones in between lie wholly
//                  inside the word.
//                  A bin that closes inside the wave's stretch and is not the stretch's first is complete: one lane writes it with plain
//                  stores.  The stretch's first and last bin may be shared with the neighbouring waves (a bin wider than a stretch: with
//                  many of them) and go through integer atomics, ONE lane per wave and bin after the wave's own reduction; integer
//                  atomics commute, so the bins are bit-reproducible.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "depth_kernels.hip.h"

#define DBNC_FN __host__ __device__ __forceinline__
#include "depth_bins_core.h"

namespace covdb {

using dbnc::Bin;
using dbnc::Partial;
using dbnc::u32;
using dbnc::u64;

__global__ __launch_bounds__(256) void k_bins_init(Bin *__restrict__ bins, u64 n) {
    const u64 i = (u64)blockIdx.x * 256ull + threadIdx.x;
    if (i < n) bins[i] = dbnc::empty_bin();
}

__device__ __forceinline__ Partial shfl_up(const Partial &p, u32 d) {
    Partial o;
    o.bin = __shfl_up(p.bin, d); o.min = __shfl_up(p.min, d); o.max = __shfl_up(p.max, d); o.covered = __shfl_up(p.covered, d);
    o.sum = __shfl_up(p.sum, d);
    return o;
}
__device__ __forceinline__ Partial shfl_lane(const Partial &p, int lane) {
    Partial o;
    o.bin = __shfl(p.bin, lane); o.min = __shfl(p.min, lane); o.max = __shfl(p.max, lane); o.covered = __shfl(p.covered, lane);
    o.sum = __shfl(p.sum, lane);
    return o;
}

// One lane leaves a bin's value: `shared` = other waves may hold bases of the bin.  (A key at or behind n_bins belongs to words without a
// base at the chunk's end and carries nothing.)
__device__ __forceinline__ void emit(Bin *__restrict__ bins, u32 n_bins, const Partial &p, bool shared) {
    if (p.bin >= n_bins) return;
    Bin *b = bins + p.bin;
    if (shared) {
        atomicAdd(reinterpret_cast<unsigned long long *>(&b->sum), (unsigned long long)p.sum);
        atomicMin(&b->min, p.min);
        atomicMax(&b->max, p.max);
        atomicAdd(&b->covered, p.covered);
    } else {
        Bin v;
        v.sum = p.sum; v.min = p.min; v.max = p.max; v.covered = p.covered; v.reserved = 0u;
        *b = v;
    }
}

__global__ __launch_bounds__(256) void k_depth_bins(const int32_t *__restrict__ arena, const u32 *__restrict__ mask, const u32 *__restrict__ rank,
                                                    const u32 *__restrict__ woff, const u32 *__restrict__ bin_off, u32 words, u32 B, Bin *__restrict__ bins,
                                                    u32 n_bins) {
    const u32 lane = threadIdx.x & 63u;
    const u64 base64 = ((u64)blockIdx.x * 4ull + (threadIdx.x >> 6)) * dbnc::STRETCH_WORDS;
    if (base64 >= words) return;      // (the whole wave)
    const u32 base = (u32)base64;
    const int4 pad4 = make_int4(dprc::PAD, dprc::PAD, dprc::PAD, dprc::PAD);
    auto load = [&](u32 w) { return w < words ? *reinterpret_cast<const int4 *>(arena + 4ull * w) : pad4; };      // the arena and every word in it are 16-byte aligned
    Partial C = dbnc::identity(0u);      // the bin open behind the step in front, the same in every lane
    u32 first = 0u;                      // the stretch's first bin
    int4 nxt = load(base + lane);
#pragma unroll 1
    for (u32 j = 0; j < dbnc::WAVE_STEPS; j++) {
        const u32 w0 = base + 64u * j;
        if (w0 >= words) break;
        const u32 w = w0 + lane;
        const int4 x4 = nxt;
        if (j + 1u < dbnc::WAVE_STEPS) nxt = load(w + 64u);
        Partial P[4];
        u32 n = 0u, key = n_bins;
        if (w < words) {
            const int32_t d[4] = {x4.x, x4.y, x4.z, x4.w};
            n = dbnc::word_of_arena(d, mask, rank, woff, bin_off, w, B, P, key);
        }
        if (n == 0u) { P[0] = dbnc::identity(key); n = 1u; }
        if (n >= 3u) emit(bins, n_bins, P[1], false);      // wholly inside the word
        if (n == 4u) emit(bins, n_bins, P[2], false);
        Partial head = P[0];
        if (j == 0u) { first = __shfl(key, 0); C = dbnc::identity(first); }
        if (lane == 0u) {
            if (C.bin == key) head = dbnc::merge(head, C);
            else emit(bins, n_bins, C, C.bin == first);
        }
        Partial S = head;      // the lane's last partial (copies by value: a choice between the array's elements would keep it in memory)
        if (n == 2u) S = P[1];
        if (n == 3u) S = P[2];
        if (n == 4u) S = P[3];
#pragma unroll
        for (u32 d = 1u; d < 64u; d <<= 1) {
            const Partial o = shfl_up(S, d);
            if (lane >= d && o.bin == S.bin) S = dbnc::merge(S, o);
        }
        const Partial front = shfl_up(S, 1u);
        if (n >= 2u) {      // the lane's first bin ends in its word
            if (lane >= 1u && front.bin == key) head = dbnc::merge(head, front);
            emit(bins, n_bins, head, key == first);
        }
        const u32 next_key = __shfl_down(key, 1u);
        if (lane < 63u && next_key != S.bin) emit(bins, n_bins, S, S.bin == first);
        C = shfl_lane(S, 63);
    }
    if (lane == 0u) emit(bins, n_bins, C, true);
}

}  // namespace covdb
