// Per-gene read aggregates (--gff; genes.rs:206-304, 493-524; covh_gene_coverage's record pass): what can be said without a wave, written
// once, run two ways (the kernels of csrc/gene_kernels.hip.h; serially on the CPU in aggregates_cpu below, which tests/c/gene_reads_host.cpp
// runs against a restatement of the reference written in the test).
//
//   classify      one record -> skip | take | nm_missing | nm_badtype, the primary bit, mism = NM.saturating_sub(indels) and the read's
//                 identity: the tests of covh_gene_coverage's record pass in their order (the reader stage's single-read branch with its
//                 f32 expressions when filter_single, then the flag filter, then unmapped, then the NM requirement).
//   verdict keys  the reference stops at the FIRST non-skipped record, in file order, that breaks a rule; at one record an NM error comes
//                 before "tid < last tid", that before "tid outside the header".  key = record index << 2 | rule: the minimum over all
//                 offending records is the verdict.
//   boundaries    a gene [s, e) takes the taken records of its contig with s <= start < e: lo / hi = lower_bound of s / e over the
//                 contig's slice of the starts (pos sign-extended to 64 bits, as the host compares them).
//   checkpoints   sum_identity = P[hi] - P[lo], P the SERIAL f64 running sum over the contig's taken records.  P is kept at every CK-th
//                 record of a contig with genes; ck_base says where a contig's checkpoints lie in one array shared by all of them.
#pragma once
#include <stdint.h>

#ifndef GNRC_FN
#define GNRC_FN inline
#endif

namespace gnrc {

typedef unsigned int u32;
typedef unsigned long long u64;

enum : u32 { SKIP = 0u, TAKE = 1u, NM_MISSING = 2u, NM_BADTYPE = 3u };
enum : u32 { RULE_NM_MISSING = 0u, RULE_NM_BADTYPE = 1u, RULE_UNSORTED = 2u, RULE_BAD_TID = 3u };
constexpr u64 NO_VERDICT = ~0ull;
constexpr u32 CK = 1024u;      // records between two checkpoints of P (a multiple of the wave: a checkpoint is a block start)

struct Filter {      // cov_config's filter fields
    u32 include_improper_pairs, include_supplementary, include_secondary, filter_single, min_mapq, min_aligned_length;
    float min_percent_identity, min_aligned_percent;
};

struct Class { u32 state, primary; u64 mism; double ident; };

// aligned = M + = + X + I + D, indels = I + D (genes.rs:258-282)
GNRC_FN void cigar_add(u32 word, u64 &aligned, u64 &indels) {
    const u32 op = word & 15u, len = word >> 4;
    if (op == 0u || op == 7u || op == 8u) aligned += len;
    else if (op == 1u || op == 2u) { aligned += len; indels += len; }
}

GNRC_FN Class classify(const Filter &f, u32 flag, u32 mapq, u32 nm_kind, u32 nm, u32 l_seq, u64 aligned, u64 indels) {
    Class c; c.state = SKIP; c.primary = 0u; c.mism = 0ull; c.ident = 0.0;
    const bool supp = (flag & 0x800u) != 0u, sec = (flag & 0x100u) != 0u, unmapped = (flag & 0x4u) != 0u;
    const u32 nm_state = nm_kind == 0u ? NM_MISSING : NM_BADTYPE;      // when nm_kind != 1 (COV_NM_UNSIGNED)
    if (f.filter_single) {      // reader stage, single-read branch (filter.rs:88-116, 243-279)
        if (unmapped || (!f.include_supplementary && supp) || (!f.include_secondary && sec)) return c;
        if (f.min_mapq != 255u && (mapq < f.min_mapq || mapq == 255u)) return c;
        if (nm_kind != 1u) { c.state = nm_state; return c; }
        const u32 al = (u32)aligned;      // u32 accumulation in the reference
        const float a = (float)al;
        if (!(al >= f.min_aligned_length && a / (float)l_seq >= f.min_aligned_percent && 1.0f - (float)nm / a >= f.min_percent_identity)) return c;
    }
    if ((!f.include_secondary && sec) || (!f.include_supplementary && supp) || (!f.include_improper_pairs && !(flag & 0x2u))) return c;
    if (unmapped) return c;
    if (nm_kind != 1u) { c.state = nm_state; return c; }
    const u64 edit = nm;
    c.state = TAKE;
    c.primary = (!supp && !sec) ? 1u : 0u;
    c.mism = edit > indels ? edit - indels : 0ull;      // saturating_sub, genes.rs:296
    c.ident = (c.primary && aligned > 0ull) ? ((double)aligned - (double)edit) / (double)aligned : 0.0;
    return c;
}

GNRC_FN u64 verdict_key(u64 record, u32 rule) { return (record << 2) | rule; }
// A taken record against the taken record in front of it (prev_tid = -2 in front of the first: host_coverage.cpp's last_tid):
// NO_VERDICT, or the key of the rule it breaks.
GNRC_FN u64 order_verdict(u64 record, int32_t tid, int32_t prev_tid, u32 n_targets) {
    if (tid == prev_tid) return NO_VERDICT;
    if (tid < prev_tid) return verdict_key(record, RULE_UNSORTED);
    if (tid < 0 || (u32)tid >= n_targets) return verdict_key(record, RULE_BAD_TID);
    return NO_VERDICT;
}

GNRC_FN u64 start_of(int32_t pos) { return (u64)(long long)pos; }

// first index in [lo, hi) whose start is >= key (hi when none): lower_bound / Rust's partition_point(|&x| x < key)
GNRC_FN u32 lower_bound_start(const int32_t *pos, u32 lo, u32 hi, u64 key) {
    while (lo < hi) {
        const u32 mid = lo + (hi - lo) / 2u;
        if (start_of(pos[mid]) < key) lo = mid + 1u; else hi = mid;
    }
    return lo;
}
// first index in [lo, hi) whose tid is >= key; tids ascend (the order rule held)
GNRC_FN u32 lower_bound_tid(const int32_t *tid, u32 lo, u32 hi, long long key) {
    while (lo < hi) {
        const u32 mid = lo + (hi - lo) / 2u;
        if ((long long)tid[mid] < key) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

// Checkpoints of the k-th contig with genes (k counts those contigs in ascending tid order) whose slice of the taken records begins at
// cs: slots ck_base .. ck_base + len / CK (checkpoint m = P in front of the slice's record m * CK).  Slices do not overlap and
// floor(a) + floor(b) <= floor(a + b), so neither do the slots; ck_slots bounds them all.
GNRC_FN u64 ck_base(u32 cs, u32 k) { return (u64)(cs / CK) + k; }
GNRC_FN u64 ck_slots(u32 n_taken, u32 n_contigs_with_genes) { return (u64)(n_taken / CK) + n_contigs_with_genes + 1ull; }

struct Aggregate { u64 n_reads, mismatches; double sum_identity; u64 contig_taken; };
struct Interval { u32 tid, pad; u64 start, end; };

// The whole computation serially.  Scratch, n entries each (n + 1 for the two integer prefixes): t_tid, t_pos, t_ident (the taken records in
// file order), p_before (P in front of each), pprim, pmism.  Returns NO_VERDICT or the verdict key; *sorted = starts never decrease inside a
// contig (0: `out` was not written).
GNRC_FN u64 aggregates_cpu(const Filter &f, u32 n_targets, u32 n, const int32_t *tid, const int32_t *pos, const uint16_t *flag, const uint8_t *mapq,
                           const u32 *nm, const uint8_t *nm_kind, const u32 *l_seq, const u32 *cigar_off, const u32 *cigar, const Interval *iv, u64 n_iv,
                           int want_identity, int32_t *t_tid, int32_t *t_pos, double *t_ident, double *p_before, u64 *pprim, u64 *pmism, Aggregate *out,
                           u64 *mapped_total, int *sorted) {
    u64 verdict = NO_VERDICT;
    u32 T = 0;
    int32_t prev = -2;
    double S = 0.0;
    *sorted = 1;
    pprim[0] = 0; pmism[0] = 0;
    for (u32 i = 0; i < n; i++) {
        u64 aligned = 0, indels = 0;
        for (u32 c = cigar_off[i]; c < cigar_off[i + 1]; c++) cigar_add(cigar[c], aligned, indels);
        const Class c = classify(f, flag[i], mapq[i], nm_kind[i], nm[i], l_seq[i], aligned, indels);
        if (c.state == SKIP) continue;
        const u64 key = c.state != TAKE ? verdict_key(i, c.state == NM_MISSING ? RULE_NM_MISSING : RULE_NM_BADTYPE) : order_verdict(i, tid[i], prev, n_targets);
        if (key < verdict) verdict = key;
        if (c.state != TAKE) continue;
        if (tid[i] != prev) S = 0.0;      // P starts again with every contig (genes.rs:500)
        else if (T != 0u && start_of(pos[i]) < start_of(t_pos[T - 1])) *sorted = 0;
        prev = tid[i];
        t_tid[T] = tid[i]; t_pos[T] = pos[i]; t_ident[T] = want_identity ? c.ident : 0.0; p_before[T] = S;
        S += t_ident[T];
        pprim[T + 1] = pprim[T] + c.primary; pmism[T + 1] = pmism[T] + c.mism;
        T++;
    }
    if (mapped_total) *mapped_total = pprim[T];
    if (verdict != NO_VERDICT || !*sorted) return verdict;
    for (u64 g = 0; g < n_iv; g++) {
        const u32 cs = lower_bound_tid(t_tid, 0, T, (long long)iv[g].tid), ce = lower_bound_tid(t_tid, cs, T, (long long)iv[g].tid + 1);
        const u32 lo = lower_bound_start(t_pos, cs, ce, iv[g].start), hi = lower_bound_start(t_pos, cs, ce, iv[g].end);
        out[g].n_reads = pprim[hi] - pprim[lo]; out[g].mismatches = pmism[hi] - pmism[lo]; out[g].contig_taken = ce - cs;
        // P[r] in front of record r: 0 at the slice's start, else the one rounded addition that made it
        const double p_lo = lo == cs ? 0.0 : p_before[lo - 1] + t_ident[lo - 1], p_hi = hi == cs ? 0.0 : p_before[hi - 1] + t_ident[hi - 1];
        out[g].sum_identity = p_hi - p_lo;
    }
    return verdict;
}

}  // namespace gnrc
