// cov_depth_runs_*: the per-base depth of a chunk of whole targets, run-length encoded on the device.  The arithmetic and the chunk's
// layout are csrc/depth_runs_core.h (shared with the CPU emulation of tests/c/depth_runs_host.cpp); the pileup that fills the arena is the
// one cov_copy_depth uses (k_pileup_stream<false, true> with depth_out / depth_off / tile_base).
//
//   k_depth_marks     a target per thread: its start bit in the mask (one bit per word of four bases), the PAD entries behind its last
//                     base, and its arena offset for the pileup
//   RankCount / RankSink      shared scan #1 over the mask's words: rank[i] = target starts in front of mask word i
//   WordCount / WordEmit      shared scan #2 over the arena's words: a lane takes four bases with one 16-byte load and the entry in front
//                     of them with one more (the scan hands a thread 16 consecutive items, so the neighbouring lane holds the word 64
//                     bases on, not the one in front; the extra entry lies in the cache line the lane has just read); the functor counts
//                     the word's run starts, the sink writes them at the word's exclusive prefix.  The output order is the scan's: target
//                     order, then position order; no atomic takes part in it.
//   ClassWordCount / ClassWordEmit      the same pair behind a view that maps every entry to its depth class (csrc/depth_class_core.h):
//                     cov_depth_class_runs_compute.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "scan_ops.hip.h"

#define DPRC_FN __host__ __device__ __forceinline__
#define DBNC_FN __host__ __device__ __forceinline__      // (depth_class_core.h brings the bins' and regions' cores with it)
#define DRGC_FN __host__ __device__ __forceinline__
#define DCLC_FN __host__ __device__ __forceinline__
#include "depth_class_core.h"

namespace covdr {

using dprc::u32;
using dprc::u64;

__global__ __launch_bounds__(256) void k_depth_marks(int32_t *__restrict__ arena, const u32 *__restrict__ woff, const u32 *__restrict__ tlen, u32 n,
                                                     u32 *__restrict__ mask, u64 *__restrict__ depth_off) {
    const u32 k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    const u32 w = woff[k];
    atomicOr(mask + (w >> 5), 1u << (w & 31u));
    dprc::mark_pads(arena, woff, tlen, k);
    depth_off[k] = 4ull * w;
}

struct RankCount { const u32 *mask; __device__ u32 operator()(u32 i) const { return dprc::popc32(mask[i]); } };
struct RankSink { u32 *rank; __device__ void operator()(u32 i, u32 p) const { rank[i] = p; } };

struct Word { int4 d; int32_t prev; bool ts; };
__device__ __forceinline__ Word load_word(const int32_t *__restrict__ arena, const u32 *__restrict__ mask, u32 w) {
    Word x;
    x.d = *reinterpret_cast<const int4 *>(arena + 4ull * w);      // the arena and every word in it are 16-byte aligned
    x.prev = w ? arena[4ull * w - 1ull] : dprc::PAD;
    x.ts = dprc::word_starts_target(mask, w);
    return x;
}

// The functors take what they compare and emit through a VIEW of the arena's entries (depth_runs_core.h): dprc::Identity for the runs of equal
// depth, dclc::ClassView (the cut list by value: scalar registers) for the runs of equal depth class.  The view is an (empty, for Identity)
// base, so the plain pair's kernel arguments are the pointers alone.
template <class View> struct WordCountT : View {
    const int32_t *arena; const u32 *mask;
    __device__ u32 operator()(u32 w) const {
        const View &q = *this;
        const Word x = load_word(arena, mask, w);
        return dprc::popc32(dprc::run_starts(q(x.d.x), q(x.d.y), q(x.d.z), q(x.d.w), q(x.prev), x.ts));      // (a view keeps PAD)
    }
};
template <class View> struct WordEmitT : View {      // dprc::emit_word over registers
    const int32_t *arena; const u32 *mask, *rank, *woff; dprc::Run *runs; u32 *run_off;
    __device__ void operator()(u32 w, u32 p) const {
        const View &q = *this;
        const Word x = load_word(arena, mask, w);
        const int32_t d[4] = {q(x.d.x), q(x.d.y), q(x.d.z), q(x.d.w)};
        const u32 m = dprc::run_starts(d[0], d[1], d[2], d[3], q(x.prev), x.ts);
        if (!x.ts && !m) return;
        const u32 k = dprc::target_of(mask, rank, w);
        if (x.ts) run_off[k] = p;
        const u32 base = 4u * (w - woff[k]);
#pragma unroll
        for (u32 j = 0; j < 4u; j++)
            if (m >> j & 1u) { dprc::Run r; r.start = base + j; r.depth = d[j]; runs[p++] = r; }
    }
};
typedef WordCountT<dprc::Identity> WordCount;
typedef WordEmitT<dprc::Identity> WordEmit;
typedef WordCountT<dclc::ClassView> ClassWordCount;
typedef WordEmitT<dclc::ClassView> ClassWordEmit;

}  // namespace covdr
