// cov_sam_*: SAM text decoded on the device, one window of raw text at a time, into the session's record store.
//
//   k_sam_masks      structure in one coalesced pass: every lane loads 16 bytes (one dwordx4), compares them with '\n' and '\t', four lanes
//                    fold their 16-bit masks into one 64-bit word with three shuffles; per 64 input bytes one word of each mask is written
//   covsc::k_scan_*  lines: popcount of the newline words, the device-wide exclusive scan of scan_ops.hip.h (the one the pair filter, the
//                    store gather and the grouping use), whose consumer (LineEmit) writes every line's end offset at the line's index
//   k_sam_count      a lane per line: record or not (empty, header), well formed or not, number of CIGAR words.  Tabs come from the tab
//                    masks, so SEQ and QUAL are jumped over, not walked.  Errors: min over (line index, code), never a race between lanes
//   covsc::k_scan_*  twice: records before each line, CIGAR words before each line
//   k_sam_decode     a lane per line: every field into the store's columns, CIGAR words at their scanned offset; with mates the
//                    next_refID and covn::name_hash of QNAME (name_hash_core.h) — the very function k_bam_extract calls
// The arithmetic is sam_parse_core.h's (shared with the CPU emulation, tests/c/sam_parse_host.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SAMC_FN __host__ __device__ __forceinline__
#include "sam_parse_core.h"
#include "scan_ops.hip.h"

namespace covs {

typedef unsigned long long u64;
typedef unsigned int u32;

// result words of one window (device, zeroed / preset before the window's kernels)
enum { RES_LINES = 0, RES_RECORDS = 1, RES_CIGAR = 2, RES_ERR = 3, RES_FIRST_REC = 4, RES_LAST_AT = 5, RES_WORDS = 8 };

// text: n bytes, readable up to the next multiple of MASK_WG_BYTES.  nl / tab: one word per 64 bytes, ceil(n / 64) of them.
__global__ __launch_bounds__(256) void k_sam_masks(const uint8_t *__restrict__ text, u64 n, u64 *__restrict__ nl, u64 *__restrict__ tab) {
    const u64 g = (u64)blockIdx.x * samc::MASK_WG + threadIdx.x, base = g * samc::LANE_BYTES;
    const uint4 q = *reinterpret_cast<const uint4 *>(text + base);
    const u32 v[4] = {q.x, q.y, q.z, q.w};
    u32 mn = samc::lane_mask16(v, (uint8_t)'\n'), mt = samc::lane_mask16(v, (uint8_t)'\t');
    const u32 keep = base >= n ? 0u : (n - base >= samc::LANE_BYTES ? 0xffffu : (1u << (u32)(n - base)) - 1u);
    mn &= keep; mt &= keep;
    const u64 wn = samc::word_of_lanes(mn, __shfl_down(mn, 1), __shfl_down(mn, 2), __shfl_down(mn, 3));
    const u64 wt = samc::word_of_lanes(mt, __shfl_down(mt, 1), __shfl_down(mt, 2), __shfl_down(mt, 3));
    if ((threadIdx.x & 3u) == 0u && base < n) { nl[g >> 2] = wn; tab[g >> 2] = wt; }
}

struct NlPop { const u64 *nl; __device__ u32 operator()(u32 w) const { return samc::popc64(nl[w]); } };
struct LineEmit {      // line p ends at the p-th newline of the window
    const u64 *nl; u32 *line_end;
    __device__ void operator()(u32 w, u32 p) const { for (u64 m = nl[w]; m; m &= m - 1ull) line_end[p++] = w * 64u + samc::ctz64(m); }
};

struct Lines { const uint8_t *text; const u64 *tab; const u32 *line_end; u32 n_lines; };
__device__ __forceinline__ void line_of(const Lines &L, u32 i, u32 &start, u32 &n) {
    start = i ? L.line_end[i - 1] + 1u : 0u;
    n = samc::trim_cr(L.text + start, L.line_end[i] - start);
}

// cnt[i] = n_cigar << 1 | is_record
__global__ __launch_bounds__(256) void k_sam_count(Lines L, u32 *__restrict__ cnt, u64 *__restrict__ res) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= L.n_lines) return;
    u32 start, n;
    line_of(L, i, start, n);
    const uint8_t *p = L.text + start;
    if (n && p[0] == '@') { cnt[i] = 0u; atomicMax(&res[RES_LAST_AT], (u64)i + 1ull); return; }      // a header line: legal in front of the first record only
    const samc::MaskTabs T{L.tab, start, n};
    const samc::LineCount c = samc::count_line(p, n, T);
    cnt[i] = (c.n_cigar << 1) | c.is_record;
    if (c.is_record) atomicMin(&res[RES_FIRST_REC], (u64)i);
    if (c.err) atomicMin(&res[RES_ERR], ((u64)i << 8) | c.err);      // the first offending line in file order, whichever lane gets here first
}

struct IsRec { const u32 *cnt; __device__ u32 operator()(u32 i) const { return cnt[i] & 1u; } };
struct NCig { const u32 *cnt; __device__ u32 operator()(u32 i) const { return cnt[i] >> 1; } };
struct Put { u32 *o; __device__ void operator()(u32 i, u32 p) const { o[i] = p; } };

struct Out {
    int32_t *tid, *pos, *mtid; uint16_t *flag; uint8_t *mapq, *nm_kind; u32 *nm, *l_seq, *cigar_off, *cigar; u64 *qh1; u32 *qh2;
    u64 rec0, cig0;
};
__global__ __launch_bounds__(256) void k_sam_decode(Lines L, const u32 *__restrict__ cnt, const u32 *__restrict__ rec_idx, const u32 *__restrict__ cig_idx, samc::Table names, Out O) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= L.n_lines || !(cnt[i] & 1u)) return;
    u32 start, n;
    line_of(L, i, start, n);
    const uint8_t *p = L.text + start;
    const samc::MaskTabs T{L.tab, start, n};
    const u64 r = O.rec0 + rec_idx[i], c = O.cig0 + cig_idx[i];
    samc::Rec R;
    samc::parse_line(p, n, T, names, R, O.cigar + c);
    O.tid[r] = R.tid; O.pos[r] = R.pos; O.flag[r] = (uint16_t)R.flag; O.mapq[r] = (uint8_t)R.mapq; O.nm[r] = R.nm; O.nm_kind[r] = (uint8_t)R.nm_kind;
    O.l_seq[r] = R.l_seq; O.cigar_off[r] = (u32)c;
    if (O.mtid) {
        O.mtid[r] = R.mtid;
        u64 k1; u32 k2;
        samc::qname_hash(p, R, k1, k2);
        O.qh1[r] = k1; O.qh2[r] = k2;
    }
}

}  // namespace covs
