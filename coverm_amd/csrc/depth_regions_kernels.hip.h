// cov_depth_regions_*: sum, min, max and covered bases of the per-base depth over arbitrary [start, end) regions (a BED file), reduced on
// the device from the chunk's arena (depth_arena_stage; the start mask and rank are not read here).  The arithmetic is
// csrc/depth_regions_core.h, shared with the CPU emulation of tests/c/depth_regions_host.cpp.
//
//   k_depth_regions  one WAVE per piece (at most dbnc::STRETCH_WORDS words of one region).  The wave finds its region by a binary search over
//                    piece_off, the same in every lane (scalar loads), reads the region's 16-byte descriptor and walks the piece in
//                    dbnc::WAVE_STEPS steps of 64 words: lane i of step j loads word w_lo + q * STRETCH_WORDS + 64 j + i with one 16-byte
//                    load (the wave reads a contiguous KiB per instruction, the next step's word is in flight while this one is reduced).
//                    A load is issued only for a word inside the region's word range: nothing is read behind the region's last word, so
//                    never behind the arena.  Every lane keeps its own partial over the steps; a piece belongs to one region, so ONE wave
//                    reduction (six shuffle rounds) follows at the end and lane 0 leaves the value: a region of one piece is complete and
//                    is written with plain stores, a region of several pieces goes through the integer atomics of covdb::emit into the
//                    value k_bins_init left.  Integer atomics commute: the result is bit-reproducible.
//                    (Regions overlap freely: each is reduced from the arena on its own, nothing is shared between two of them.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "depth_bins_kernels.hip.h"

#define DRGC_FN __host__ __device__ __forceinline__
#include "depth_regions_core.h"

namespace covrg {

using dbnc::Bin;
using dbnc::Partial;
using dbnc::u32;
using dbnc::u64;

__global__ __launch_bounds__(256) void k_depth_regions(const int32_t *__restrict__ arena, const drgc::Desc *__restrict__ desc, const u32 *__restrict__ piece_off,
                                                       u32 n_regions, u32 n_pieces, Bin *__restrict__ out) {
    const u32 lane = threadIdx.x & 63u;
    const u32 p = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));      // the wave's piece (the launch keeps it below 2^32)
    if (p >= n_pieces) return;      // (the whole wave)
    const u32 r = drgc::region_of_piece(piece_off, n_regions, p);
    const drgc::Desc d = desc[r];
    const u32 n_of = drgc::pieces_of(d), q = p - piece_off[r];
    const u32 i0 = drgc::piece_begin(q), i1 = drgc::piece_end(d, q);      // the piece's words inside the region
    const int32_t *__restrict__ base = arena + 4ull * d.w_lo;            // the region's first word; the arena and every word in it are 16-byte aligned
    // The word travels as ONE 128-bit integer: as a vector of four the compiler takes the load apart into four conditional 4-byte loads.
    // (A word outside [i0, i1) holds no base of the region and is never added: it is not loaded.)
    typedef unsigned __int128 word_t;
    auto load = [&](u32 i) { return i < i1 ? *reinterpret_cast<const word_t *>(base + 4ull * i) : (word_t)0; };
    Partial P = dbnc::identity(r);
    word_t nxt = load(i0 + lane);
#pragma unroll 1
    for (u32 j = 0; j < dbnc::WAVE_STEPS; j++) {
        const u32 w0 = i0 + 64u * j;
        if (w0 >= i1) break;      // (the whole wave)
        const u32 i = w0 + lane;
        const word_t x = nxt;
        if (j + 1u < dbnc::WAVE_STEPS) nxt = load(i + 64u);
        if (i < i1) drgc::add_word(P, d, i, (int32_t)(u32)x, (int32_t)(u32)(x >> 32), (int32_t)(u32)(x >> 64), (int32_t)(u32)(x >> 96));
    }
#pragma unroll
    for (u32 s = 32u; s >= 1u; s >>= 1) {
        Partial o;
        o.bin = r; o.min = __shfl_down(P.min, s); o.max = __shfl_down(P.max, s); o.covered = __shfl_down(P.covered, s); o.sum = __shfl_down(P.sum, s);
        if (lane + s < 64u) P = dbnc::merge(P, o);
    }
    if (lane == 0u) covdb::emit(out, n_regions, P, n_of > 1u);
}

}  // namespace covrg
