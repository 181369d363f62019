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
//   k_depth_regions_thr  the same walk which also counts, per threshold of cov_depth_thresholds_set, the region's bases at or above it
//                    (csrc/depth_class_core.h); see regions_body.
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

// THR: the threshold variant (cov_depth_thresholds_set).  The same walk, the same single load; the word's entries outside the region become PAD
// (dclc::mask_word), and per threshold t and entry the lanes' compare d >= thr[t] is ONE lane mask whose bits are counted on the scalar side
// (ballot, popcount, add: scalar registers) — no per-lane counter, no vector register per threshold and no wave reduction for the counts.
// The list is a kernel argument by value and the loop over it is unrolled behind a uniform test, so thr.c[t] and cnt[t] have constant indices.
template <bool THR>
__device__ __forceinline__ void regions_body(const int32_t *__restrict__ arena, const drgc::Desc *__restrict__ desc, const u32 *__restrict__ piece_off,
                                             u32 n_regions, u32 n_pieces, Bin *__restrict__ out, const dclc::Cuts &thr, u32 *__restrict__ counts) {
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
    u32 cnt[dclc::MAX_CUTS] = {};      // (THR) the piece's counts, the same in every lane; a piece has at most dbnc::STRETCH_BASES bases
    word_t nxt = load(i0 + lane);
#pragma unroll 1
    for (u32 j = 0; j < dbnc::WAVE_STEPS; j++) {
        const u32 w0 = i0 + 64u * j;
        if (w0 >= i1) break;      // (the whole wave)
        const u32 i = w0 + lane;
        const word_t x = nxt;
        if (j + 1u < dbnc::WAVE_STEPS) nxt = load(i + 64u);
        if (i < i1) drgc::add_word(P, d, i, (int32_t)(u32)x, (int32_t)(u32)(x >> 32), (int32_t)(u32)(x >> 64), (int32_t)(u32)(x >> 96));
        if constexpr (THR) {
            int32_t e[4] = {(int32_t)(u32)x, (int32_t)(u32)(x >> 32), (int32_t)(u32)(x >> 64), (int32_t)(u32)(x >> 96)};
            dclc::mask_word(d, i, e);
#pragma unroll
            for (u32 k = 0; k < 4u; k++) e[k] = i < i1 ? e[k] : dprc::PAD;      // (a lane behind the piece holds the zero word, not a base)
#pragma unroll
            for (u32 t = 0; t < dclc::MAX_CUTS; t++) {
                if (t < thr.n) {      // (the whole wave)
#pragma unroll
                    for (u32 k = 0; k < 4u; k++) cnt[t] += (u32)__popcll(__ballot(e[k] >= thr.c[t]));
                }
            }
        }
    }
#pragma unroll
    for (u32 s = 32u; s >= 1u; s >>= 1) {
        Partial o;
        o.bin = r; o.min = __shfl_down(P.min, s); o.max = __shfl_down(P.max, s); o.covered = __shfl_down(P.covered, s); o.sum = __shfl_down(P.sum, s);
        if (lane + s < 64u) P = dbnc::merge(P, o);
    }
    if (lane == 0u) covdb::emit(out, n_regions, P, n_of > 1u);
    if constexpr (THR) {
        // row r of the chunk's counts: a region of one piece is complete (plain stores), a region of several adds into the zero fill
        // (integer adds commute: the bytes are the same on every run)
        if (lane == 0u) {
            u32 *__restrict__ row = counts + (u64)r * thr.n;
#pragma unroll
            for (u32 t = 0; t < dclc::MAX_CUTS; t++) {
                if (t < thr.n) {
                    if (n_of > 1u) atomicAdd(row + t, cnt[t]); else row[t] = cnt[t];
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_depth_regions(const int32_t *__restrict__ arena, const drgc::Desc *__restrict__ desc, const u32 *__restrict__ piece_off,
                                                       u32 n_regions, u32 n_pieces, Bin *__restrict__ out) {
    regions_body<false>(arena, desc, piece_off, n_regions, n_pieces, out, dclc::Cuts{}, nullptr);
}
// counts: n_regions x thr.n, row-major, zero-filled by the caller; thr.n >= 1.
__global__ __launch_bounds__(256) void k_depth_regions_thr(const int32_t *__restrict__ arena, const drgc::Desc *__restrict__ desc, const u32 *__restrict__ piece_off,
                                                           u32 n_regions, u32 n_pieces, Bin *__restrict__ out, const dclc::Cuts thr, u32 *__restrict__ counts) {
    regions_body<true>(arena, desc, piece_off, n_regions, n_pieces, out, thr, counts);
}

}  // namespace covrg
