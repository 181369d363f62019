// Host instantiation of csrc/finish_plan_core.h beside the decisions as finish_once took them before they had one owner: each where the pass
// first needed it, in the order and under the conditions it stood there (frozen below, the expressions written out as they stood, the session's
// fields replaced by the facts).  Test infrastructure (tests/test_finish_plan_core.py builds it with g++, as a library for the comparisons
// and as a program — main below walks the same grid — for a run under the sanitizers); not part of the product.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "../../coverm_amd/csrc/finish_plan_core.h"

typedef unsigned int u32;
typedef unsigned long long u64;
constexpr int PREP_PASSES = 8;      // pileup_kernels.hip.h

// What the test compares, as plain integers (the order of FIELDS in tests/test_finish_plan_core.py).
struct Flat {
    u64 long_cigars, prep_passes, prep_chunk, prep_grid, n_steps, gen_all, gen_grid, est_lanes, run_prep, prep7, run_pileup, identity_side,
        id_primary, id_nonsupp, compacted, derive_in_est, hist_stats_launch, hist_prefetch, nf, runs, genomes, genome_identity, lean_error, ncig,
        want_hist, want_id, lean, genome_lanes_from;
};
constexpr int N_FIELDS = sizeof(Flat) / sizeof(u64);

static Flat flat_of(const finplan::FinishPlan &p) {
    return Flat{p.long_cigars, (u64)p.prep_passes, p.prep_chunk, p.prep_grid, p.n_steps, p.gen_all, p.gen_grid, p.est_lanes, p.run_prep, p.prep7,
                p.run_pileup, p.identity_side, p.id_primary, p.id_nonsupp, p.compacted, p.derive_in_est, p.hist_stats_launch, p.hist_prefetch,
                p.nf, p.runs, p.genomes, p.genome_identity, p.lean_without_genomes, p.ncig, p.want_hist, p.want_id, p.lean, p.genome_lanes_from};
}

// finish_once as it stood: only the lines that decide, in their order; `s->x` became `F.x`, a launch or a branch became the flag that says it ran.
static Flat frozen(const finplan::Facts &F) {
    Flat o;
    memset(&o, 0, sizeof o);
    const bool lean = F.lean_finish;
    const u32 nT = F.nT;
    const u32 R = F.R;
    const bool want_hist = F.want & COV_WANT_HIST, want_id = F.want & COV_WANT_IDENTITY;
    bool compacted = false;
    bool derive_in_est = false;
    const bool est_lanes = F.est_lanes_knob < 0 ? nT >= 65536u : F.est_lanes_knob == 1;
    const uint64_t ncig_all = F.ncig;
    const bool long_cigars = R && ncig_all / R >= 16;
    const int prep_kernel = F.prep_kernel;
    const int prep_passes = long_cigars ? 1 : 2 * PREP_PASSES, prep_b = 1;
    const u32 prep_chunk = (u32)(256 * prep_b * prep_passes);
    const u32 prep_grid = (R + prep_chunk - 1) / prep_chunk;
    o.id_nonsupp = want_id && !(F.want & COV_WANT_IDENTITY_PRIMARY_ONLY);      // d_ident is reserved, idn is not NULL
    o.id_primary = want_id && !(F.want & COV_WANT_IDENTITY_NONSUPP_ONLY);      // d_identp is reserved, idp is not NULL
    if (R) {
        o.run_prep = 1;
        const u32 n_steps = (R + 63u) / 64u;
        const bool gen_all = prep_kernel != 7 && (uint64_t)R < (uint64_t)nT * 128u;
        const u32 gen_grid = gen_all ? std::min<u32>((u32)F.n_cus * 64u, (n_steps + 3u) / 4u) : std::min<u32>((u32)F.n_cus * 8u, (n_steps + 3u) / 4u);
        o.n_steps = n_steps; o.gen_all = gen_all; o.gen_grid = gen_grid;
        if (want_id && nT) o.identity_side = 1;
    }
    o.prep7 = prep_kernel == 7;      // (COV_LAUNCH_PREP's first branch; the plan says which kernel would run also when none does)
    if (R && F.n_tiles) {
        o.run_pileup = 1;
        compacted = want_hist && (F.est_n == 0 || F.hist_fetch_seen);
        derive_in_est = want_hist && !compacted && !(F.have_mask || F.have_runs) && F.est_n != 0;
        if (want_hist && !derive_in_est) o.hist_stats_launch = 1;
        if (want_hist) {
            if (compacted) {
                const bool guess = F.hist_fetch_seen;      // (the size of the copy is the session's state; whether there is one is decided here)
                if (guess) o.hist_prefetch = 1;
            }
        }
    }
    const size_t nf = (F.have_mask || F.have_runs) ? 0 : (size_t)nT * F.est_n;
    if (want_id && R && nT) o.identity_side |= 2;      // the join in front of the estimators: the same condition a second time
    const bool runs = F.have_runs && F.est_n != 0 && !F.spill_active && !F.in_spill;
    const bool genomes = runs || (F.have_genomes && F.est_n != 0 && !F.spill_active && !F.in_spill);
    if (lean && !genomes) o.lean_error = 1;
    o.genome_identity = want_id && !(F.want & (runs ? COV_WANT_IDENTITY_NONSUPP_ONLY : COV_WANT_IDENTITY_PRIMARY_ONLY));
    o.long_cigars = long_cigars; o.prep_passes = (u64)prep_passes; o.prep_chunk = prep_chunk; o.prep_grid = prep_grid; o.est_lanes = est_lanes;
    o.compacted = compacted; o.derive_in_est = derive_in_est; o.nf = nf; o.runs = runs; o.genomes = genomes; o.ncig = ncig_all;
    o.want_hist = want_hist; o.want_id = want_id; o.lean = lean;
    // stage_genomes as it stood: `const bool lanes = nG >= 65536u;` — the count it compared nG with; the knob (new with the plan's field)
    // replaces the count by "always" / "never"
    o.genome_lanes_from = F.est_lanes_knob < 0 ? 65536u : F.est_lanes_knob == 1 ? 0u : 0xffffffffu;
    // the side stream's launch and its join always came together
    if (o.identity_side == 1 || o.identity_side == 2) o.identity_side = ~0ull;
    else o.identity_side = o.identity_side == 3;
    return o;
}

static finplan::Facts facts_of(u32 R, u32 nT, u32 n_tiles, u64 ncig, u32 want, u32 est_n, int knob, int prep_kernel, int n_cus, u32 flags) {
    finplan::Facts f;
    f.R = R; f.nT = nT; f.n_tiles = n_tiles; f.ncig = ncig; f.want = want; f.est_n = est_n; f.est_lanes_knob = knob; f.prep_kernel = prep_kernel; f.n_cus = n_cus;
    f.have_mask = flags & 1; f.have_runs = flags & 2; f.have_genomes = flags & 4; f.spill_active = flags & 8; f.in_spill = flags & 16;
    f.lean_finish = flags & 32; f.hist_fetch_seen = flags & 64;
    return f;
}

extern "C" {
int finplan_n_fields(void) { return N_FIELDS; }
void finplan_plan(uint32_t R, uint32_t nT, uint32_t n_tiles, uint64_t ncig, uint32_t want, uint32_t est_n, int knob, int prep_kernel, int n_cus, uint32_t flags, uint64_t *out) {
    const Flat o = flat_of(finplan::plan(facts_of(R, nT, n_tiles, ncig, want, est_n, knob, prep_kernel, n_cus, flags)));
    memcpy(out, &o, sizeof o);
}
void finplan_frozen(uint32_t R, uint32_t nT, uint32_t n_tiles, uint64_t ncig, uint32_t want, uint32_t est_n, int knob, int prep_kernel, int n_cus, uint32_t flags, uint64_t *out) {
    const Flat o = frozen(facts_of(R, nT, n_tiles, ncig, want, est_n, knob, prep_kernel, n_cus, flags));
    memcpy(out, &o, sizeof o);
}
}

// The grid: every threshold of the plan from both sides, every combination of the want bits and of the boolean facts.
// seen[v][k]: field k was zero (v = 0) / not zero (v = 1) somewhere.  Returns the cases walked.
static u64 walk(u64 *bad_out, u64 seen[2][N_FIELDS]) {
    const u32 Rs[] = {0, 1, 63, 64, 65, 1279, 1280, 1281, 4096, 4097, 0xffffffefu}, nTs[] = {0, 1, 10, 65535, 65536}, tiles[] = {0, 1, 1025};
    const int knobs[] = {-1, 0, 1}, preps[] = {0, 7}, cus[] = {1, 256};
    u64 n = 0, bad = 0;
    for (u32 R : Rs) for (u32 nT : nTs) for (u32 nt : tiles) for (int cw = 0; cw < 3; cw++) for (u32 est_n = 0; est_n < 2; est_n++)
    for (int knob : knobs) for (int pk : preps) for (int cu : cus) for (u32 want = 0; want < 16; want++) for (u32 flags = 0; flags < 128; flags++, n++) {
        const u64 ncig = cw == 0 ? 15ull * R : cw == 1 ? (R ? 16ull * R - 1 : 0) : 16ull * R;
        const finplan::Facts f = facts_of(R, nT, nt, ncig, want, est_n, knob, pk, cu, flags);
        const Flat a = flat_of(finplan::plan(f)), b = frozen(f);
        if (memcmp(&a, &b, sizeof a)) bad++;
        u64 w[N_FIELDS]; memcpy(w, &a, sizeof a);
        for (int k = 0; k < N_FIELDS; k++) seen[w[k] != 0][k] = 1;
    }
    *bad_out = bad;
    return n;
}

extern "C" uint64_t finplan_walk(uint64_t *bad, uint64_t *seen) {
    u64 sn[2][N_FIELDS] = {}, b = 0;
    const u64 n = walk(&b, sn);
    *bad = b; memcpy(seen, sn, sizeof sn);
    return n;
}

int main() {
    u64 seen[2][N_FIELDS] = {}, bad = 0;
    const u64 n = walk(&bad, seen);
    for (int k = 0; k < N_FIELDS; k++) if (!seen[1][k]) bad++;      // every field is set somewhere on the grid
    printf("%llu cases, %llu bad\n", n, bad);
    return bad ? 1 : 0;
}
