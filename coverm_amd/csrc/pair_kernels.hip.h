// Reader-stage PAIR filter on the device: ReferenceSortedBamFilter::read, pair branch
// (src/filter.rs:117-228) with filter_out = true, over the session's own record store as the device ingest filled it
// (k_bam_extract keeps next_refID and a 96-bit hash of the read name when the session asks for mates).
//
// What the reference does, record by record: among primary proper-pair records (:133-146) it keeps a set of "first" records of
// the current reference keyed by read name, emptied whenever the reference changes (:149-161); a record whose name is not in the
// set is parked there if its mate maps to the same reference (:170-176); a record whose name is in the set takes its partner out,
// the pair is judged (:188-207: the single-read predicate on both when single thresholds are set, then read_pair_passes_filter
// :281-336) and, if it passes, the FIRST record is returned followed by the SECOND (:208-217).
//
// Here: a per-(reference, name) hash join.  Records are sorted by reference (the ingest verified that their keys never decrease,
// else the file goes to the CPU reader), so "the set of the current reference" is "the records with this tid" and chunks of
// whole references are independent.  Per chunk:
//   k_pair_insert    every eligible record finds / claims the table entry of its (tid, name hash) and leaves its index there
//                    (lowest, highest, count) — no order dependence, no locks
//   k_pair_resolve   every entry with exactly two records is one candidate pair (first = lower index, second = higher): parked
//                    only if the first's mate reference is this reference, then judged with the reference's own f32 expressions;
//                    partner[second] = first.  An entry with more than two records (a read name that occurs three or more times
//                    among the primary proper-pair records of one reference) needs the serial park / take-out sequence: counted
//                    per chunk; for such chunks k_pair_collect lists the members of those entries, the host replays the sequence
//                    over the (short) sorted list and k_pair_judge_list judges the candidate pairs it yields.  Only a file with
//                    more than 2^20 such records goes to the CPU reader.
// The output order is the reference's: pairs in the order of their SECOND records, first record then second — an exclusive scan
// over partner[] gives every pair its two output slots (k_scan_*), and k_pair_gather* builds the selected record store.
//
// Name hashes: 96 bits (MurmurHash3-x86-128-style mixing, three of its four words) + the tid compared in full; two different
// names of one reference collide with probability ~n^2 / 2^97, 10^-13 for 2*10^8 records.  The claim protocol (two 64-bit
// compare-and-swaps per entry) never merges different keys whatever the interleaving.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "name_hash_core.h"
#include "pair_key_core.h"

namespace covp {

typedef unsigned long long u64;
typedef unsigned int u32;

constexpr u32 NONE = 0xffffffffu;

struct PairEntry {     // 32 B, all-zero = empty
    u64 k1;            // name hash words 0-1 (never 0)
    u64 k2t;           // name hash word 2 | (tid + 2) << 32 (never 0)
    u32 nlo;           // max over the entry's records of ~index: lowest index = ~nlo
    u32 hi;            // highest index
    u32 cnt, pad;
};

struct PairCols {
    const int32_t *tid; const uint16_t *flag; const uint8_t *mapq, *nm_kind;
    const u32 *nm, *l_seq, *cigar_off, *cigar;
    const int32_t *mtid; const u64 *qh1; const u32 *qh2;
};

struct PairFilter {    // cov_pair_filter (covermhip.h)
    int32_t filter_single;
    uint8_t min_mapq, pad[3];
    u32 min_aligned_length_single;
    float min_percent_identity_single, min_aligned_percent_single;
    u32 min_aligned_length_pair;
    float min_percent_identity_pair, min_aligned_percent_pair;
};

__device__ __forceinline__ bool eligible(u32 flag) { return !(flag & 0x900u) && (flag & 0x2u); }     // filter.rs:133-146

// Primary records of the whole store (filter.rs:129-131 counts them before any test).
__global__ __launch_bounds__(256) void k_count_primary(const uint16_t *__restrict__ flag, u32 n, u64 *__restrict__ out) {
    u32 c = 0;
    for (u32 i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) c += (flag[i] & 0x900u) ? 0u : 1u;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, (u64)c);
}

// cuts[c], c = 0 .. n_chunks: chunk c = records [cuts[c], cuts[c + 1]) — whole references only: the cut for target c * T is the
// first record whose key exceeds the key of record c * T - 1 (binary search: keys never decrease).
__device__ __forceinline__ u32 key_of(int32_t tid) { return tid < 0 ? 0x7fffffffu : (u32)tid; }
__global__ void k_pair_cuts(const int32_t *__restrict__ tid, u32 n, u32 T, u32 n_chunks, u32 *__restrict__ cuts) {
    const u32 c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > n_chunks) return;
    if (c == 0) { cuts[0] = 0; return; }
    if (c == n_chunks || (u64)c * T >= n) { cuts[c] = n; return; }
    const u32 k = key_of(tid[c * T - 1]);
    u32 lo = c * T, hi = n;               // first index in [lo, hi] with key > k
    while (lo < hi) { const u32 mid = lo + (hi - lo) / 2; if (key_of(tid[mid]) > k) hi = mid; else lo = mid + 1; }
    cuts[c] = lo;
}

// The key of a record and the slot its probe run starts at: csrc/pair_key_core.h (one statement for the kernels, the driver and the CPU test)
using pkey::key_k1; using pkey::key_k2t; using pkey::table_slot;

__global__ __launch_bounds__(256) void k_pair_insert(PairCols C, u32 r0, u32 r1, PairEntry *__restrict__ T, u32 mask, u32 *__restrict__ counters) {
    const u32 i = r0 + blockIdx.x * 256u + threadIdx.x;
    if (i >= r1) return;
    if (!eligible(C.flag[i])) return;
    const u64 k1 = key_k1(C.qh1[i]), k2t = key_k2t(C.qh2[i], C.tid[i]);
    u32 h = table_slot(k1, k2t, mask);
    for (u32 probe = 0; probe <= mask; probe++, h = (h + 1u) & mask) {
        PairEntry *e = T + h;
        const u64 p1 = atomicCAS(&e->k1, 0ull, k1);
        if (p1 != 0ull && p1 != k1) continue;
        // the entry carries my first word (mine or an equal one): whoever sets the second word first owns it; a different key with
        // an equal first word moves on to the next slot, and so does every later record of that key
        const u64 p2 = atomicCAS(&e->k2t, 0ull, k2t);
        if (p2 != 0ull && p2 != k2t) continue;
        atomicMax(&e->nlo, ~i); atomicMax(&e->hi, i); atomicAdd(&e->cnt, 1u);
        return;
    }
    atomicAdd(counters + 1, 1u);      // table full: the host sized it at twice the chunk, so this is a bug, reported as such
}

__device__ __forceinline__ u32 aligned_of(const PairCols &C, u32 i, bool with_del) {
    u32 a = 0;
    for (u32 c = C.cigar_off[i], e = C.cigar_off[i + 1]; c < e; c++) {
        const u32 w = C.cigar[c], op = w & 15u, len = w >> 4;
        if (op == 0u || op == 1u || op == 7u || op == 8u || (with_del && op == 2u)) a += len;
    }
    return a;
}

// One candidate pair (first record i1 parked, second record i2 arrived): the reference's judgement (filter.rs:188-207), with its
// short-circuit order; first_err: lowest (second index << 8 | COV_ERR_NM_* code) over the pairs whose judgement needed a missing NM.
__device__ __forceinline__ void judge_pair(const PairCols &C, const PairFilter &f, u32 i1, u32 i2, u32 *__restrict__ partner, u64 *__restrict__ first_err,
                                           u32 err_missing, u32 err_badtype) {
    u32 err = 0;
    auto nm = [&](u32 i, u64 &v) -> bool {    // lib.rs:138-158: the reference panics; here the first such record in file order is reported
        const u32 k = C.nm_kind[i];
        if (k == 1u) { v = C.nm[i]; return true; }
        if (!err) err = k == 0u ? err_missing : err_badtype;
        return false;
    };
    auto single_ok = [&](u32 i) -> bool {     // filter.rs:243-279
        const u32 mq = C.mapq[i];
        if (f.min_mapq != 255 && (mq < f.min_mapq || mq == 255u)) return false;
        u64 ed;
        if (!nm(i, ed)) return false;
        const u32 al = aligned_of(C, i, true);
        return al >= f.min_aligned_length_single && (float)al / (float)C.l_seq[i] >= f.min_aligned_percent_single &&
               1.0f - (float)ed / (float)al >= f.min_percent_identity_single;
    };
    bool pass = !f.filter_single || (single_ok(i1) && single_ok(i2));
    if (pass) {                                // filter.rs:281-336 (record = second, record1 = first)
        const u32 m1 = C.mapq[i1], m2 = C.mapq[i2];
        if (f.min_mapq != 255 && (m1 < f.min_mapq || m2 < f.min_mapq || m1 == 255u || m2 == 255u)) pass = false;
        else {
            u64 e2, e1;
            if (!nm(i2, e2) || !nm(i1, e1)) pass = false;
            else {
                const u64 ed = e2 + e1;
                const u32 al = aligned_of(C, i2, false) + aligned_of(C, i1, false);
                pass = al >= f.min_aligned_length_pair && (float)al / (float)((u64)C.l_seq[i1] + C.l_seq[i2]) >= f.min_aligned_percent_pair &&
                       1.0f - (float)ed / (float)al >= f.min_percent_identity_pair;
            }
        }
    }
    if (err) atomicMin(first_err, ((u64)i2 << 8) | (u64)err);
    if (pass) partner[i2] = i1;
}

// counters: [1] table overflow; multi[chunk]: entries of this chunk with more than two records
__global__ __launch_bounds__(256) void k_pair_resolve(PairCols C, const PairEntry *__restrict__ T, u32 n_entries, PairFilter f, u32 *__restrict__ partner,
                                                      u32 *__restrict__ multi, u64 *__restrict__ first_err, u32 err_missing, u32 err_badtype) {
    const u32 g = blockIdx.x * 256u + threadIdx.x;
    if (g >= n_entries) return;
    const PairEntry e = T[g];
    if (e.cnt < 2u) return;
    if (e.cnt > 2u) { atomicAdd(multi, 1u); return; }
    const u32 i1 = ~e.nlo, i2 = e.hi;
    if (C.mtid[i1] != C.tid[i1]) return;      // the first record was not parked (filter.rs:170-176); the second then finds nothing
    judge_pair(C, f, i1, i2, partner, first_err, err_missing, err_badtype);
}

// Members of the entries with more than two records: (entry, record index, would this record be parked).  n_list counts every
// member even when the list is full (the host then knows it was).
struct MultiRec { u32 entry, i, parks, pad; };
__global__ __launch_bounds__(256) void k_pair_collect(PairCols C, u32 r0, u32 r1, const PairEntry *__restrict__ T, u32 mask, MultiRec *__restrict__ list, u32 cap,
                                                      u32 *__restrict__ n_list) {
    const u32 i = r0 + blockIdx.x * 256u + threadIdx.x;
    if (i >= r1) return;
    if (!eligible(C.flag[i])) return;
    const u64 k1 = key_k1(C.qh1[i]), k2t = key_k2t(C.qh2[i], C.tid[i]);
    u32 h = table_slot(k1, k2t, mask);
    for (u32 probe = 0; probe <= mask; probe++, h = (h + 1u) & mask) {
        const PairEntry e = T[h];
        if (e.k1 == 0ull) return;              // (cannot happen: every eligible record of the chunk was inserted)
        if (e.k1 != k1 || e.k2t != k2t) continue;
        if (e.cnt > 2u) {
            const u32 slot = atomicAdd(n_list, 1u);
            if (slot < cap) { MultiRec m; m.entry = h; m.i = i; m.parks = C.mtid[i] == C.tid[i] ? 1u : 0u; m.pad = 0; list[slot] = m; }
        }
        return;
    }
}
__global__ __launch_bounds__(256) void k_pair_judge_list(PairCols C, const uint2 *__restrict__ pairs, u32 n, PairFilter f, u32 *__restrict__ partner,
                                                         u64 *__restrict__ first_err, u32 err_missing, u32 err_badtype) {
    const u32 g = blockIdx.x * 256u + threadIdx.x;
    if (g >= n) return;
    judge_pair(C, f, pairs[g].x, pairs[g].y, partner, first_err, err_missing, err_badtype);
}

// ---------------------------------------------------------------------------------------------- items and consumers of the device-wide scan (scan_ops.hip.h)
struct PairSlots { const u32 *partner; __device__ u32 operator()(u32 i) const { return partner[i] != NONE ? 2u : 0u; } };
struct PairEmit {      // order[p] = first, order[p + 1] = second
    const u32 *partner; u32 *order;
    __device__ void operator()(u32 i, u32 p) const { const u32 a = partner[i]; if (a != NONE) { order[p] = a; order[p + 1] = i; } }
};
struct SelCigarLen { const u32 *order, *cigar_off; __device__ u32 operator()(u32 p) const { const u32 j = order[p]; return cigar_off[j + 1] - cigar_off[j]; } };

struct Store {
    int32_t *tid, *pos; uint16_t *flag; uint8_t *mapq, *nm_kind; u32 *nm, *l_seq, *cigar_off, *cigar;
};
// Consumer of the CIGAR-length scan: writes the selected record p (fixed fields, its new CIGAR offset, its CIGAR words).
struct SelGather {
    const u32 *order; Store src, dst;
    __device__ void operator()(u32 p, u32 coff) const {
        const u32 j = order[p];
        dst.tid[p] = src.tid[j]; dst.pos[p] = src.pos[j]; dst.flag[p] = src.flag[j]; dst.mapq[p] = src.mapq[j]; dst.nm_kind[p] = src.nm_kind[j];
        dst.nm[p] = src.nm[j]; dst.l_seq[p] = src.l_seq[j]; dst.cigar_off[p] = coff;
        const u32 c0 = src.cigar_off[j], n = src.cigar_off[j + 1] - c0;
        for (u32 k = 0; k < n; k++) dst.cigar[coff + k] = src.cigar[c0 + k];
    }
};

// 96-bit hash of a read name: csrc/name_hash_core.h (one function for the BGZF extraction, the SAM text decode and the CPU emulation)
using covn::name_hash;

}  // namespace covp
