// The decisions of one pass of the device pipeline over the record store (finish_once in covermhip.hip): which kernels run, on which side,
// and what sizes their launches — taken once, right after the argument check, from the facts below; the stages of the pass read the plan and
// never a decision's inputs.  Arithmetic only, no HIP: tests/c/finish_plan_host.cpp runs it on the CPU against the expressions finish_once
// carried while it took each decision where it first needed it.
#pragma once
#include <algorithm>

#include "../../include/covermhip.h"

namespace finplan {
typedef unsigned int u32;
typedef unsigned long long u64;

constexpr int LEAN_PASSES = 16;      // 2 x PREP_PASSES (pileup_kernels.hip.h; pinned by a static_assert in covermhip.hip)

struct Facts {
    u32 R = 0, nT = 0, n_tiles = 0;      // records in the store, targets, tiles of all targets
    u64 ncig = 0;                        // CIGAR words of the store (of the adopted batch)
    u32 want = 0, est_n = 0;             // cov_config::want, estimators set
    int est_lanes_knob = -1, prep_kernel = 0, n_cus = 256;
    bool have_mask = false, have_runs = false, have_genomes = false;
    bool spill_active = false, in_spill = false, lean_finish = false, hist_fetch_seen = false;
};

struct FinishPlan {
    bool want_hist = false, want_id = false, lean = false;
    u64 ncig = 0;
    // k_prep geometry: 4096 records per workgroup for short reads (k_prep_lean: each of the four waves walks 16 steps of 64 consecutive records;
    // k_prep7s: 16 passes of 256); one step / pass when CIGARs are long, where the work per record is large and records are few (long-read
    // mappings), so that every CU gets workgroups
    bool run_prep = false, prep7 = false;      // there are records; COVERM_PREP_KERNEL=7: k_prep7s, the second implementation
    bool long_cigars = false;
    int prep_passes = LEAN_PASSES, prep_b = 1;
    u32 prep_chunk = 0, prep_grid = 0;
    // k_prep_lean's loop takes the steps of 64 records that lie inside one contig; a sample with fewer than ~128 records per contig has few
    // of those, and k_prep_generic then walks every step itself (no list, no partial records for k_post_prep to add)
    u32 n_steps = 0, gen_grid = 0;
    bool gen_all = false;
    bool est_lanes = false;              // an assembly: a lane per contig (pileup_kernels.hip.h, estimate_body)
    // the genome entries' count is the pass's own when the separator scan builds them (stage 9), so the plan holds the count from which
    // a lane per genome runs (genome_kernels.hip.h, genome_estimate_body): 65 536 as for the contigs, the knob forces it on (0) / off
    u32 genome_lanes_from = 65536u;
    bool run_pileup = false;             // scans, ranges, histogram layout, pileup: there are records and tiles
    bool identity_side = false;          // the identity kernels run on the side stream, beside k_ranges / k_pileup
    bool id_primary = false, id_nonsupp = false;      // identity streams actually needed (the others: skipped by k_prep and the k_id_* kernels)
    // With the histogram wanted the pileup leaves the bins and cov_out; the contigs' window statistics are derived from the bins once
    // per contig (hist_stats_derive): by the estimator kernel as its prologue when it is the first reader — no launch added —, else
    // by k_hist_stats, in front of k_hist_sum<1> / the genome and separator kernels / the copy of the result block.
    bool compacted = false;              // the compact histogram is built by this pass (else: by the first cov_fetch_hist)
    bool derive_in_est = false;          // the estimator kernel derives the statistics (else k_hist_stats did, or there are none)
    bool hist_stats_launch = false;
    bool hist_prefetch = false;          // the compact histogram's copy to the host starts inside the pass: the caller fetched the last one
    // (with a target mask the entries are genomes — aggregated when cov_set_genomes gave their table, else by the caller: masked-out
    // contigs have no bins in the arena, and nobody may fetch per-contig floats — no k_estimate launch, no floats in the copy)
    u64 nf = 0;
    // genome entries: not after a spill — the contigs that left the store are on the host, the caller aggregates there
    bool runs = false, genomes = false, genome_identity = false;
    bool lean_without_genomes = false;   // status: cov_finish_genomes with nothing to aggregate on the device (COV_ERR_STATE)
};

inline FinishPlan plan(const Facts &f) {
    FinishPlan p;
    const u32 R = f.R, nT = f.nT;
    const bool want_hist = f.want & COV_WANT_HIST, want_id = f.want & COV_WANT_IDENTITY;
    p.want_hist = want_hist; p.want_id = want_id; p.lean = f.lean_finish; p.ncig = f.ncig;
    p.run_prep = R != 0; p.prep7 = f.prep_kernel == 7;
    p.est_lanes = f.est_lanes_knob < 0 ? nT >= 65536u : f.est_lanes_knob == 1;
    p.genome_lanes_from = f.est_lanes_knob < 0 ? 65536u : f.est_lanes_knob == 1 ? 0u : ~0u;
    p.long_cigars = R && f.ncig / R >= 16;
    p.prep_passes = p.long_cigars ? 1 : LEAN_PASSES;
    p.prep_chunk = (u32)(256 * p.prep_b * p.prep_passes);
    p.prep_grid = (R + p.prep_chunk - 1) / p.prep_chunk;
    p.id_primary = want_id && !(f.want & COV_WANT_IDENTITY_NONSUPP_ONLY);
    p.id_nonsupp = want_id && !(f.want & COV_WANT_IDENTITY_PRIMARY_ONLY);
    if (R) {
        p.n_steps = (R + 63u) / 64u;
        p.gen_all = f.prep_kernel != 7 && (u64)R < (u64)nT * 128u;
        p.gen_grid = p.gen_all ? std::min<u32>((u32)f.n_cus * 64u, (p.n_steps + 3u) / 4u) : std::min<u32>((u32)f.n_cus * 8u, (p.n_steps + 3u) / 4u);      // waves stride over the steps
        p.identity_side = want_id && nT;
    }
    p.run_pileup = R && f.n_tiles;
    if (p.run_pileup) {
        p.compacted = want_hist && (f.est_n == 0 || f.hist_fetch_seen);
        p.derive_in_est = want_hist && !p.compacted && !(f.have_mask || f.have_runs) && f.est_n != 0;
        p.hist_stats_launch = want_hist && !p.derive_in_est;
        p.hist_prefetch = p.compacted && f.hist_fetch_seen;
    }
    p.nf = (f.have_mask || f.have_runs) ? 0 : (u64)nT * f.est_n;
    p.runs = f.have_runs && f.est_n != 0 && !f.spill_active && !f.in_spill;
    p.genomes = p.runs || (f.have_genomes && f.est_n != 0 && !f.spill_active && !f.in_spill);
    p.genome_identity = want_id && !(f.want & (p.runs ? COV_WANT_IDENTITY_NONSUPP_ONLY : COV_WANT_IDENTITY_PRIMARY_ONLY));
    p.lean_without_genomes = p.lean && !p.genomes;
    return p;
}
}  // namespace finplan
